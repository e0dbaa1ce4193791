"""The write-footprint checker itself (tests/helpers.py: Guarded), on CPU tensors: it passes on a correctly written interior, fails
when one guard byte is flipped, and fails when one interior element is left at the sentinel -- or written where it must not be."""
import numpy as np
import pytest
import torch

from helpers import GUARD_ALIGN, GUARD_TILE, Guarded, sentinel_bits

DTYPES = (torch.float32, torch.float64, torch.uint8, torch.int32)
SHAPES = (((130,), -1), ((12, 130), -1), ((3, 12, 65), -1), ((2, 130, 14), 1), ((7, 3, 1), -1))


def _fill(g):
    g.interior.copy_(torch.arange(g.interior.numel()).reshape(g.shape) % 5)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("shape,n_axis", SHAPES, ids=lambda v: str(v))
def test_layout_and_sentinels(dtype, shape, n_axis):
    g = Guarded("x", shape, dtype, n_axis=n_axis, device="cpu")
    n = shape[n_axis]
    row = n * int(np.prod(shape[n_axis % len(shape) + 1:], dtype=np.int64))
    assert g.interior.shape == shape and g.interior.is_contiguous() and g.interior.dtype == dtype
    assert g.interior.data_ptr() % GUARD_ALIGN == 0
    assert g.front >= row                                                   # one row in front
    n_up = -(-n // GUARD_TILE) * GUARD_TILE
    assert g.raw.numel() - g.front - g.numel >= g.numel // n * n_up + row   # the array at whole tiles plus one row behind
    # the documented bit patterns, byte for byte
    want = {torch.float32: bytes.fromhex("A5A5C57F"), torch.float64: bytes.fromhex("A5A5A5A5A5A5F87F"), torch.uint8: b"\xA5",
            torch.int32: b"\xA5\xA5\xA5\xA5"}[dtype]
    assert bytes(g.raw.view(torch.uint8)[:len(want)].tolist()) == want
    assert bool(g.untouched().all())
    g.check(written=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_passes_on_written_interior(dtype):
    g = Guarded("x", (3, 12, 130), dtype, device="cpu")
    _fill(g)
    assert g.check() is g.interior


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("where", ("front-first", "front-last", "back-first", "back-last"))
def test_fails_on_one_flipped_guard_byte(dtype, where):
    g = Guarded("x", (12, 130), dtype, device="cpu")
    _fill(g)
    raw = g.raw.view(torch.uint8)
    item = g.raw.element_size()
    at = {"front-first": 0, "front-last": g.front * item - 1, "back-first": (g.front + g.numel) * item, "back-last": raw.numel() - 1}[where]
    raw[at] ^= 1
    with pytest.raises(AssertionError, match="guard overwritten"):
        g.check()
    raw[at] ^= 1
    g.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_fails_on_one_unwritten_element(dtype):
    g = Guarded("x", (12, 130), dtype, device="cpu")
    _fill(g)
    g.bits()[11, 129] = sentinel_bits(dtype)[1]
    with pytest.raises(AssertionError, match="never written"):
        g.check()


def test_partial_write_mask():
    """`written` as a mask: exactly those elements are written (final_obs: the auto-reset envs only)."""
    g = Guarded("final_obs", (12, 130), torch.float32, device="cpu")
    mask = torch.arange(130) % 3 == 0
    g.interior[:, mask] = 1.0
    g.check(written=mask)
    with pytest.raises(AssertionError, match="must stay untouched"):
        g.check(written=False)
    g.interior[5, 1] = 0.0
    with pytest.raises(AssertionError, match="must stay untouched"):
        g.check(written=mask)


def test_nan_payload_is_not_confused_with_other_nans():
    """Bit patterns are compared, not isnan: a kernel that stores an ordinary NaN has written the element."""
    g = Guarded("x", (130,), torch.float64, device="cpu")
    g.interior.fill_(float("nan"))
    g.check()
