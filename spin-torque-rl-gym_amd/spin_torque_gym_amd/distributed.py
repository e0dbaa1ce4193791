"""Multi-GPU: one process per GPU, contiguous shards of independent environments, one collective per step.

The reference has no distributed path at all; this is a new design for the 8-GPU MI355X node.
Environments never interact, so the data path needs no exchange: rank r owns envs [r*n_local, (r+1)*n_local) and steps
them with its own `stg_ctx` (Philox counters use the GLOBAL env index, so results do not depend on the number of ranks).
The only communication is what an RL learner needs -- the step's (obs, reward, terminated, truncated) of every env.

Copy-free by layout.  The step kernel writes its outputs as 56-byte env-major RECORDS (`out_layout='records'`,
include/spintorque_hip.h: STG_OUT_RECORDS) straight into the collective's send buffer -- a shard's records are one
contiguous block -- and ONE all-gather (RCCL over xGMI when the backend is "nccl"; the CPU tests run the same code over
gloo) assembles the GLOBAL record array uint8[N_global, 56]; what the learner gets are typed strided VIEWS of that array --
obs float32 [N_global, 12] (Gym's orientation), reward float32 [N_global], terminated / truncated bool [N_global].  No
staging copy before the collective, no transposition or `torch.cat` after it.  Two send buffers and two global arrays
alternate, so the gather of step k runs on its own HIP stream under the kernel of step k+1 (`gather_begin` /
`gather_end`), which writes the other pair.  At 131 072 envs per GPU a rank contributes 7.3 MB per step.
(`inplace=True` makes the send buffer this rank's slice of the global array itself -- NCCL/RCCL's in-place all-gather
form; the point-to-point exchange always works that way.)

`gather_algo`: "all_gather" (default) = `all_gather_into_tensor`, RCCL picks the algorithm; "p2p" = one grouped batch of
7 sends + 7 receives per rank (`batch_isend_irecv`), every peer's slice over its own xGMI link at once -- the one-shot
alternative to a ring (ring = 7 hops per link-time, direct = 1), for steps short enough that the
collective no longer hides under the kernel; it is also what ragged shards (num_envs % world != 0) use, since it does not
need equal contributions.

Actions go the other way: every rank slices its shard out of the global action tensor (a learner that is itself
data-parallel over the same ranks passes local actions and skips the gather: ``gather=False``).
"""
import time
from typing import Optional

import torch
import torch.distributed as dist

from .backend import RECORD_BYTES, record_views
from .envs import STATE_TENSORS, SpinTorqueVecEnv, _TimerTable, assemble_state, check_state_config, state_span


def shard_range(n_global: int, world: int, rank: int):
    """Contiguous block partition; the first (n_global % world) ranks take one extra env."""
    base, extra = divmod(n_global, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def global_views(records: torch.Tensor):
    """(obs [N,12] f32, reward [N] f32, terminated [N] bool, truncated [N] bool): strided views of a record array, no copy."""
    obs, reward, term, trunc, _ = record_views(records)
    return obs, reward, term.view(torch.bool), trunc.view(torch.bool)


def _records_behind(obs, reward, term, trunc, status) -> torch.Tensor:
    """The record array uint8 [ko, n, 56] of a SpinTorqueVecEnv.step_many in the records layout, from the obs [ko, n, 12] it returned:
    with the HIP backend that obs IS a strided view of the array the launch wrote (backend.record_views), and this is the view back,
    no copy.  A backend that hands out separate arrays instead (the CPU oracle behind the tests' backend seam) gets them packed."""
    ko, n, _ = obs.shape
    words = RECORD_BYTES // 4
    if (obs.dtype == torch.float32 and tuple(obs.stride()) == (words * n, words, 1) and obs.storage_offset() == 0
            and obs.untyped_storage().nbytes() >= ko * n * RECORD_BYTES):
        return obs.as_strided((ko, n, words), (words * n, words, 1)).view(torch.uint8)
    if obs.is_cuda:
        raise RuntimeError("step_many did not return views of a record array (out_layout='records' is what the sharded env builds)")
    rec = torch.zeros((ko, n, RECORD_BYTES), dtype=torch.uint8)
    o, r, te, tr, st = record_views(rec)
    o.copy_(obs), r.copy_(reward), te.copy_(term), tr.copy_(trunc)
    if status is not None:
        st.copy_(status)
    return rec


class ShardedSpinTorqueVecEnv:
    """`num_envs` global environments sharded over the ranks of `group` (default: the world group).  step() / step_many() advance
    every env by one / K steps per launch and gather the records; state_dict() / load_state_dict() checkpoint the shards and
    resume them under any other world size (or in a one-process SpinTorqueVecEnv)."""

    def __init__(self, num_envs: int, group: Optional[dist.ProcessGroup] = None, device_index: Optional[int] = None,
                 class_index=None, gather_algo: str = "all_gather", inplace: bool = False, overlap: Optional[bool] = None,
                 **env_kwargs):
        if env_kwargs.get("pulse_shape") is not None or env_kwargs.get("applied_field") is not None:
            raise NotImplementedError("ShardedSpinTorqueVecEnv is not implemented with pulse_shape or applied_field: shaped pulses and "
                                      "an applied field run on SpinTorqueVecEnv (step, step_many, step_ids, send / recv); the sharded "
                                      "env does not hand the shape to its shards yet")
        if env_kwargs.get("pulse_knots") is not None:
            raise NotImplementedError("ShardedSpinTorqueVecEnv is not implemented with pulse_knots: agent-shaped pulses run on "
                                      "SpinTorqueVecEnv (step, step_many, step_ids, send / recv); the sharded env does not hand the "
                                      "knots to its shards yet")
        if not dist.is_initialized():
            raise RuntimeError("torch.distributed must be initialised (backend 'nccl' = RCCL on ROCm, or 'gloo')")
        if gather_algo not in ("all_gather", "p2p"):
            raise ValueError("gather_algo must be 'all_gather' or 'p2p'")
        self.group = group
        self.gather_algo = gather_algo
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.num_envs = int(num_envs)
        self.lo, self.hi = shard_range(self.num_envs, self.world, self.rank)
        self.n_local = self.hi - self.lo
        self._spans = [shard_range(self.num_envs, self.world, r) for r in range(self.world)]
        # point-to-point operations address their peer by GLOBAL rank (torch.distributed.P2POp), shards are indexed by the
        # rank inside `group`: the two differ for any group that is not the world
        self._global = [r if group is None else dist.get_global_rank(group, r) for r in range(self.world)]
        if self.num_envs % self.world and gather_algo == "all_gather":
            # ragged shards: an all-gather needs equal contributions; the point-to-point exchange does not care
            gather_algo = self.gather_algo = "p2p"
        if device_index is None:
            device_index = self.rank % max(torch.cuda.device_count(), 1)
        if class_index is not None:
            class_index = torch.as_tensor(class_index)[self.lo:self.hi]
        env_kwargs.pop("out_layout", None)
        self.local = SpinTorqueVecEnv(self.n_local, class_index=class_index, device_index=device_index, env_id0=self.lo,
                                      out_layout="records", **env_kwargs)
        dev = self.local.backend.packed.device
        self.device = dev
        # two global record arrays: the kernel of step k writes this rank's slice of array k & 1 while the gather of
        # step k-1 (array (k-1) & 1) may still be in flight
        self._glob = [torch.zeros((self.num_envs, RECORD_BYTES), dtype=torch.uint8, device=dev) for _ in range(2)]
        # where the step kernel writes: the slice of the global array itself (p2p / in-place all-gather), or a send buffer
        # of its own (the plain out-of-place all-gather, the most travelled path through RCCL)
        self._inplace = bool(inplace) or gather_algo == "p2p"
        self._send = None if self._inplace else [torch.zeros((self.n_local, RECORD_BYTES), dtype=torch.uint8, device=dev)
                                                 for _ in range(2)]
        self._slot = 0            # array the NEXT step writes
        self._filled = None       # array holding the last step's local records, not yet gathered
        self._last = None         # ... whether gathered or not (gather_again)
        self._pending = None
        self._gloo = dist.get_backend(group) == "gloo"
        # the exchange on its own HIP stream, ordered against the step kernels by events.  Automatic: RCCL (stream-ordered
        # collectives).  Over gloo the exchange is a host-side copy out / collective / copy in and gains nothing from a side
        # stream; overlap=True still routes it through the same stream-and-event protocol (the staging copies run on the side
        # stream), which is how the protocol is tested with two processes on ONE GPU, where RCCL cannot run.
        self._overlap = dev.type == "cuda" and (not self._gloo if overlap is None else bool(overlap))
        self._done = [None, None]
        if self._overlap:
            self._comm_stream = torch.cuda.Stream(device=dev)
        self.profiler = _TimerTable()

    # -- the collective ---------------------------------------------------------------------------------------------
    def _mine(self, k: int) -> torch.Tensor:
        """The record array of slot k that this rank's step kernel writes and the exchange sends."""
        return self._glob[k][self.lo:self.hi] if self._inplace else self._send[k]

    def _exchange(self, k: int) -> None:
        """Assembles global array k from every rank's records of slot k."""
        g, mine = self._glob[k], self._mine(k)
        if self._gloo:
            # CPU tests / single-GPU rehearsal: gloo moves host memory and is not an in-place collective
            host = torch.empty(g.shape, dtype=torch.uint8)
            # (device tensors: .cpu() / copy_ run on the CURRENT stream -- the side stream when the caller is gather_begin with
            # overlap -- and block the host until that stream has reached them)
            if self.gather_algo == "p2p" and self.world > 1:
                src = mine.cpu()
                ops = []
                for peer, (plo, phi) in enumerate(self._spans):
                    if peer != self.rank:
                        ops.append(dist.P2POp(dist.isend, src, self._global[peer], group=self.group))
                        ops.append(dist.P2POp(dist.irecv, host[plo:phi], self._global[peer], group=self.group))
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
                host[self.lo:self.hi] = src
            else:
                dist.all_gather_into_tensor(host.view(-1), mine.cpu().reshape(-1), group=self.group)
            g.copy_(host)
            return
        if self.gather_algo == "p2p" and self.world > 1:
            ops = []
            for peer, (plo, phi) in enumerate(self._spans):
                if peer != self.rank:
                    ops.append(dist.P2POp(dist.isend, mine, self._global[peer], group=self.group))
                    ops.append(dist.P2POp(dist.irecv, g[plo:phi], self._global[peer], group=self.group))
            for w in dist.batch_isend_irecv(ops):
                w.wait()            # (stream-ordered on NCCL/RCCL: does not block the host)
            return
        # (in-place form: the send buffer is this rank's slice of the receive buffer, NCCL/RCCL's in-place all-gather)
        dist.all_gather_into_tensor(g.view(-1), mine.reshape(-1), group=self.group)

    def _gather(self, unpack: bool = True):
        """Synchronous form: gathers the last step's records and returns the typed global views (unpack=False: the
        global record array uint8 [N_global, 56] itself)."""
        self.gather_begin()
        return self.gather_end(unpack)

    def gather_begin(self):
        """Starts the all-gather of the step just enqueued and returns at once: the collective runs on a side stream
        (RCCL over xGMI) concurrently with whatever the caller enqueues next -- normally the next step's kernel, which
        writes the OTHER global array.  Pair with `gather_end`."""
        if self._filled is None:
            raise RuntimeError("gather_begin without a step (or reset) to gather")
        k, self._filled = self._filled, None
        t0 = time.perf_counter()
        if not self._overlap:
            self._exchange(k)
            self._pending = ("sync", k)
        else:
            cur = torch.cuda.current_stream(self.device)
            ready = torch.cuda.Event()
            ready.record(cur)                                    # the step kernel that wrote this rank's slice
            with torch.cuda.stream(self._comm_stream):
                self._comm_stream.wait_event(ready)
                self._exchange(k)
                done = torch.cuda.Event()
                done.record(self._comm_stream)
            self._done[k] = done
            self._pending = ("async", k)
        self.profiler.add("gather_begin", time.perf_counter() - t0)

    def gather_end(self, unpack: bool = True):
        """Makes the current stream wait for the gather started last; returns (obs [N,12], reward [N], terminated [N],
        truncated [N]) as views of the global record array (valid until the step after next overwrites that array), or
        the array itself with unpack=False."""
        if self._pending is None:
            raise RuntimeError("gather_end without gather_begin")
        kind, k = self._pending
        self._pending = None
        if kind == "async":
            torch.cuda.current_stream(self.device).wait_event(self._done[k])
        return global_views(self._glob[k]) if unpack else self._glob[k]

    def gather_again(self) -> None:
        """Marks the records of the last step as not yet gathered, so that gather_begin() exchanges them once more
        (measuring the collective by itself)."""
        if self._last is None:
            raise RuntimeError("nothing has been stepped yet")
        self._filled = self._last

    @property
    def gather_in_flight(self) -> bool:
        """A gather_begin() is waiting for its gather_end()."""
        return self._pending is not None

    # -- env API ----------------------------------------------------------------------------------------------------
    def _next_slot(self) -> int:
        k = self._slot
        self._slot ^= 1
        if self._overlap and self._done[k] is not None:
            # the gather that last filled this array must be through before the kernel overwrites our slice of it
            torch.cuda.current_stream(self.device).wait_event(self._done[k])
        return k

    def reset(self, seed: Optional[int] = None, options=None, gather: bool = True):
        options = dict(options or {})
        for key in ("initial_state", "target_state", "mask"):
            if options.get(key) is not None:
                v = torch.as_tensor(options[key])
                if v.dim() >= 1 and v.shape[0] == self.num_envs:
                    options[key] = v[self.lo:self.hi]
        obs, info = self.local.reset(seed=seed, options=options)
        if not gather:
            return obs, info
        # reset() fills the env's own record array (obs fields; reward/flags zeroed): hand it to the exchange
        k = self._next_slot()
        self._mine(k).copy_(self.local.backend.packed)
        self._filled = self._last = k
        return self._gather()[0], info

    def step(self, actions, gather: bool = True, actions_are_local: bool = False, actions_soa: bool = False):
        """One env.step() of this rank's shard, written into its slice of the next global record array.  gather=True
        also runs the exchange and returns the GLOBAL (obs, reward, terminated, truncated, {}); gather=False returns the
        local env's outputs (views of this rank's slice) -- follow with gather_begin()/gather_end() to pipeline."""
        a = torch.as_tensor(actions)
        if not actions_are_local:
            a = a[:, self.lo:self.hi] if actions_soa else a[self.lo:self.hi]
        k = self._next_slot()
        out = self.local.step(a, actions_soa=actions_soa, out=self._mine(k))
        self._filled = self._last = k
        if not gather:
            return out
        obs, reward, term, trunc = self._gather()
        return obs, reward, term, trunc, {}

    def scatter_actions(self, actions=None, src: int = 0, dtype=torch.float32):
        """A centralised learner's actions -> this rank's shard: `actions` [N_global, 2] on rank `src` (ignored elsewhere),
        8 B/env over the same links as the gather, in the other direction.  Returns the local [n_local, 2] tensor; pass it
        to step(..., actions_are_local=True)."""
        dev = torch.device("cpu") if self._gloo else self.device
        local = torch.empty((self.n_local, 2), dtype=dtype, device=dev)
        chunks = None
        if self.rank == src:
            a = torch.as_tensor(actions).to(device=dev, dtype=dtype)
            if tuple(a.shape) != (self.num_envs, 2):
                raise ValueError(f"expected actions of shape ({self.num_envs}, 2), got {tuple(a.shape)}")
            chunks = [a[plo:phi].contiguous() for plo, phi in self._spans]
        gsrc = self._global[src]
        if self.num_envs % self.world == 0:
            dist.scatter(local, chunks, src=gsrc, group=self.group)
            return local
        # ragged shards: one send per peer (scatter needs equal chunks)
        if self.rank == src:
            ops = [dist.P2POp(dist.isend, chunks[peer], self._global[peer], group=self.group) for peer in range(self.world) if peer != src]
            local.copy_(chunks[src])
        else:
            ops = [dist.P2POp(dist.irecv, local, gsrc, group=self.group)]
        for w in (dist.batch_isend_irecv(ops) if ops else []):
            w.wait()
        return local

    # -- K fused steps per launch ----------------------------------------------------------------------------------------
    def step_many(self, actions, out_every: bool = True, autoreset: Optional[bool] = None, gather: bool = True,
                  actions_are_local: bool = False, final_obs_out: Optional[torch.Tensor] = None):
        """K env.step()s of this rank's shard in ONE launch (SpinTorqueVecEnv.step_many in the records layout), then the exchange.
        actions: [K, N_global, 2], or [K, n_local, 2] with actions_are_local; float32 or float64 as for step().  `autoreset` must be
        the env's own convention (it is fixed at construction and part of every checkpoint); None = that.
        Returns (obs [ko, N_global, 12], reward [ko, N_global], terminated, truncated, info) with ko = K (out_every) or 1 (the last
        step only): typed strided views of ONE new record array uint8 [ko, N_global, 56], which is info['records'];
        info['status'] is its status byte and, with autoreset, info['final_obs'] float32 [ko, N_global, 12] holds the terminal
        observation of the envs whose episode ended (zero elsewhere, as in the one-process env).  The arrays are this call's own:
        they stay valid for as long as the caller holds them (the two-array ring of step() is not involved).
        final_obs_out (out_every only): a float32 [K, N_global, 12] array of the caller's that receives the terminal observations
        instead -- rows of envs that did not end at that step are left as they are; it is then info['final_obs'].
        gather=False: no exchange; the same tuple for this rank's envs only (views of the launch's own [ko, n_local, 56] output).

        Form of the exchange.  The launch writes [ko][n_local][56]: step k of this rank is one contiguous block, and so is
        out[k, lo_r:hi_r] of every rank r in the global array, but the K blocks of a rank are N_global records apart there, so
        the kernel cannot write them in place and one all-gather cannot cover all K.  Equal shards with gather_algo 'all_gather':
        ONE all_gather_into_tensor PER STEP SLICE, from the launch's block k straight into out[k] (ko collectives, enqueued back to
        back; RCCL's most travelled call).  gather_algo 'p2p', which ragged shards always use: ONE grouped batch for all K --
        ko x (world - 1) sends of block k and receives straight into out[k, lo_r:hi_r] -- plus a device copy of this rank's own
        ko blocks into its slices.  Nothing is transposed or concatenated.  final_obs travels the same way, 48 B/env.  Over gloo
        (host memory) a rank's ko blocks go through one staging tensor per peer, as the one-step exchange stages there.  The
        exchange runs on the side stream when the env overlaps; the current stream waits for it before this call returns."""
        if autoreset is not None and bool(autoreset) != self.local.autoreset:
            raise ValueError(f"autoreset={bool(autoreset)} but this env was built with autoreset={self.local.autoreset}")
        a = torch.as_tensor(actions)
        if a.dim() != 3 or a.shape[2] != 2 or a.shape[1] != (self.n_local if actions_are_local else self.num_envs):
            raise ValueError(f"expected actions [K, {self.n_local if actions_are_local else self.num_envs}, 2], got {tuple(a.shape)}")
        if not actions_are_local:
            a = a[:, self.lo:self.hi]
        K = int(a.shape[0])
        ko = K if out_every else 1
        auto = self.local.autoreset
        if final_obs_out is not None:
            if not (auto and out_every and gather):
                raise ValueError("final_obs_out needs autoreset, out_every=True (the flags that say which rows to write are per step) "
                                 "and gather=True")
            if (final_obs_out.dtype != torch.float32 or tuple(final_obs_out.shape) != (K, self.num_envs, 12)
                    or final_obs_out.device != self.device):
                raise ValueError(f"final_obs_out must be float32 [{K}, {self.num_envs}, 12] on {self.device}")
        obs, reward, term, trunc, info = self.local.step_many(a, out_every=out_every)
        if not gather:
            return obs, reward, term, trunc, info
        rec = _records_behind(obs, reward, term, trunc, info.get("status"))
        out = torch.empty((ko, self.num_envs, RECORD_BYTES), dtype=torch.uint8, device=self.device)
        pairs = [(rec, out)]
        if auto:
            fin = info["final_obs"]
            fin = fin if fin.is_contiguous() else fin.contiguous()       # (env-major [ko, n_local, 12] already in the records layout)
            fout = torch.empty((ko, self.num_envs, 12), dtype=torch.float32, device=self.device)
            pairs.append((fin.view(torch.uint8), fout.view(torch.uint8)))
        t0 = time.perf_counter()
        if not self._overlap:
            self._exchange_many(pairs)
        else:
            cur = torch.cuda.current_stream(self.device)
            ready = torch.cuda.Event()
            ready.record(cur)                                            # the launch that wrote the blocks
            with torch.cuda.stream(self._comm_stream):
                self._comm_stream.wait_event(ready)
                self._exchange_many(pairs)
                done = torch.cuda.Event()
                done.record(self._comm_stream)
            # (the arrays were allocated on the current stream; it waits here, so whatever frees or reuses them comes after)
            cur.wait_event(done)
        self.profiler.add("gather_many", time.perf_counter() - t0)
        g_obs, g_reward, g_term, g_trunc, g_status = record_views(out)
        g_term, g_trunc = g_term.view(torch.bool), g_trunc.view(torch.bool)
        g_info = {"records": out, "status": g_status}
        if auto:
            if final_obs_out is not None:
                ended = (g_term | g_trunc).unsqueeze(-1)
                final_obs_out.copy_(torch.where(ended, fout, final_obs_out))
                fout = final_obs_out
            g_info["final_obs"] = fout
        return g_obs, g_reward, g_term, g_trunc, g_info

    def _exchange_many(self, pairs) -> None:
        """For every (mine uint8 [ko, n_local, B], glob uint8 [ko, N_global, B]): glob[k, lo_r:hi_r] = rank r's mine[k]."""
        p2p = self.gather_algo == "p2p" and self.world > 1
        if self._gloo:
            for mine, g in pairs:
                ko, _, nb = mine.shape
                src = mine.cpu()
                host = torch.empty(g.shape, dtype=torch.uint8)
                if p2p:
                    # one message per peer and array (gloo matches a pair's messages in order): the peer's ko blocks, then placed
                    stage = {peer: torch.empty((ko, phi - plo, nb), dtype=torch.uint8)
                             for peer, (plo, phi) in enumerate(self._spans) if peer != self.rank}
                    ops = []
                    for peer, buf in stage.items():
                        ops.append(dist.P2POp(dist.isend, src, self._global[peer], group=self.group))
                        ops.append(dist.P2POp(dist.irecv, buf, self._global[peer], group=self.group))
                    for w in dist.batch_isend_irecv(ops):
                        w.wait()
                    for peer, buf in stage.items():
                        plo, phi = self._spans[peer]
                        host[:, plo:phi] = buf
                    host[:, self.lo:self.hi] = src
                else:
                    for k in range(ko):
                        dist.all_gather_into_tensor(host[k].view(-1), src[k].reshape(-1), group=self.group)
                g.copy_(host)
            return
        if p2p:
            ops = []
            for mine, g in pairs:
                for k in range(mine.shape[0]):
                    for peer, (plo, phi) in enumerate(self._spans):
                        if peer != self.rank:
                            ops.append(dist.P2POp(dist.isend, mine[k], self._global[peer], group=self.group))
                            ops.append(dist.P2POp(dist.irecv, g[k, plo:phi], self._global[peer], group=self.group))
                g[:, self.lo:self.hi].copy_(mine)
            for w in dist.batch_isend_irecv(ops):
                w.wait()            # (stream-ordered on NCCL/RCCL: does not block the host)
            return
        for mine, g in pairs:
            for k in range(mine.shape[0]):
                dist.all_gather_into_tensor(g[k].view(-1), mine[k].reshape(-1), group=self.group)

    # -- checkpoint / resume -------------------------------------------------------------------------------------------------
    def _end_gather(self) -> None:
        """Ends whatever the exchange has in flight and returns the slot ring to its initial state (cf. _AsyncPool.drain)."""
        if self._pending is not None:
            self.gather_end()
        if self._overlap:
            self._comm_stream.synchronize()
        self._done = [None, None]
        self._slot, self._filled, self._last = 0, None, None

    def state_dict(self, gather_to: Optional[int] = None):
        """This rank's checkpoint: SpinTorqueVecEnv.state_dict()'s keys for its own envs -- m / target [3, n_local], total_energy,
        step_count, rng_step, done [n_local] (left on the device), host_rng, cfg_seed, env_id0 (= lo) -- plus the global metadata
        n_global, world, rank, lo, hi and config (SpinTorqueVecEnv.result_config(): solver, thermal field, noise model, max_steps,
        targets, autoreset, ... -- everything that decides results).  Every rank calls it; without gather_to there is no
        communication at all (the metadata is checked against this rank's own shard only).
        gather_to=r: rank r's dict holds the full [N_global] state instead (lo, hi = 0, N_global; env_id0 = 0; one gather per
        tensor), the dict a SpinTorqueVecEnv(num_envs=N_global) saves, for writing a single file; the other ranks still get
        their per-rank dict.  load_state_dict takes either, at any world size."""
        loc = self.local
        if loc.num_envs != self.hi - self.lo or loc.env_id0 != self.lo:
            raise RuntimeError(f"shard [{self.lo}, {self.hi}) but the local env holds {loc.num_envs} envs from {loc.env_id0}")
        loc._no_pool("state_dict")
        st = dict(loc.backend.get_state())
        st.update(host_rng=loc._rng.bit_generator.state, cfg_seed=int(loc.cfg.seed), env_id0=int(self.lo),
                  n_global=self.num_envs, world=self.world, rank=self.rank, lo=self.lo, hi=self.hi, config=loc.result_config())
        if gather_to is None:
            return st
        if not 0 <= int(gather_to) < self.world:
            raise ValueError(f"gather_to must be a rank of the group, 0..{self.world - 1}")
        full = {key: self._gather_to(st[key], int(gather_to)) for key in STATE_TENSORS}
        if self.rank != int(gather_to):
            return st
        st = dict(st, **full)
        st.update(env_id0=0, lo=0, hi=self.num_envs)
        return st

    def _gather_to(self, t: torch.Tensor, dst: int):
        """One gather of a per-env tensor [..., n_local] to group rank dst: [..., N_global] there, None elsewhere.  Ragged shards
        are padded to the largest one for the collective (gather needs equal contributions)."""
        dev = torch.device("cpu") if self._gloo else self.device
        width = self._spans[0][1] - self._spans[0][0]
        mine = torch.zeros((*t.shape[:-1], width), dtype=t.dtype, device=dev)
        mine[..., :self.n_local] = t
        bufs = [torch.empty_like(mine) for _ in range(self.world)] if self.rank == dst else None
        dist.gather(mine, bufs, dst=self._global[dst], group=self.group)
        if bufs is None:
            return None
        return torch.cat([b[..., :phi - plo] for b, (plo, phi) in zip(bufs, self._spans)], dim=-1).to(self.device)

    def load_state_dict(self, st) -> None:
        """Resumes bit for bit from (a) a per-rank dict of the same world size and rank, (b) a full [N_global] dict -- state_dict(
        gather_to=...)'s or a SpinTorqueVecEnv(num_envs=N_global).state_dict() -- of which this rank slices its [lo, hi), or (c) a
        LIST of the per-rank dicts of ANY world size, of which it takes the overlaps with its [lo, hi).  An env's streams are keyed
        by (cfg_seed, global env id, rng_step), all of which travel, so the partition does not matter.  ValueError, naming the
        field: n_global or a result-deciding config field differs, or the lo, hi ranges of a list do not tile [0, n_global).
        Ends a gather in flight first.  No communication."""
        self._end_gather()
        is_list = isinstance(st, (list, tuple))
        pieces = list(st) if is_list else [st]
        for p in pieces:
            n_g = p.get("n_global")
            if n_g is None and not is_list and state_span(p)[0] == 0:
                n_g = state_span(p)[1]            # a one-process env's dict: all of its envs, from env 0
            if n_g is not None and int(n_g) != self.num_envs:
                raise ValueError(f"checkpoint has n_global={n_g}, this env has n_global={self.num_envs}")
        mine = assemble_state(pieces, self.lo, self.hi, tile=is_list)
        check_state_config(mine, self.local.result_config())
        mine.pop("config", None)
        self.local.load_state_dict(mine)

    def get_performance_stats(self):
        st = self.local.get_performance_stats()
        st["profiler"].update(self.profiler.get_stats())
        return st

    def close(self):
        self.local.close()
