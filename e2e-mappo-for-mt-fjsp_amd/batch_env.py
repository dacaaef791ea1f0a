"""DeviceBatchEnv — device-resident batch of MT-FJSP instances over the C ABI.

torch is used ONLY as plumbing (device buffers + stream handle); every computation
is a HIP kernel in libmtfjsp.so.  Method names follow the reference's
trainer/parallel_env.py so the parity tests read like the reference's call sites.
"""
import ctypes as C

import numpy as np
import torch

from . import capi


def shop_of_machine(edge):
    """reference `edge` table [B,E,M/E] (machine ids per shop, generate…py:219-233) -> [B,M] shop index."""
    edge = np.asarray(edge)
    B, E, W = edge.shape
    out = np.zeros((B, E * W), np.int32)
    for e in range(E):
        np.put_along_axis(out, edge[:, e, :].astype(np.int64), e, axis=1)
    return out


def step_kernel_for(n_job, n_machine, batch, obs_f32=False, lds_max=160 * 1024):
    """(name, instances per workgroup, bytes of one instance's LDS region, any diagnostic switch set) of the step kernel a handle of
    this shape launches where a workgroup may use `lds_max` bytes of LDS (gfx950: 160 KiB): the library's own selection, no GPU needed.
    ValueError for a shape mtfjsp_create refuses, one whose single instance needs more than `lds_max` bytes included"""
    g, nb, ov = C.c_int32(), C.c_int64(), C.c_int32()
    name = capi.lib().mtfjsp_step_kernel_name_for(n_job, n_machine, batch, int(bool(obs_f32)), lds_max, C.byref(g), C.byref(nb), C.byref(ov))
    if name is None:
        raise ValueError(f"no handle takes J{n_job}M{n_machine} B={batch} with {lds_max} bytes of LDS per workgroup")
    return name.decode(), g.value, nb.value, bool(ov.value)


def _out(x, shape, dt, dev):
    """an optional output: True -> a new tensor, None / False -> None (not computed), a tensor -> itself, to write into"""
    if x is None or x is False:
        return None
    if x is True:
        return torch.empty(shape, dtype=dt, device=dev)
    assert x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() == int(np.prod(shape))
    return x


def _ptr(x):
    return C.c_void_p(None if x is None else x.data_ptr())


class DeviceBatchEnv:
    def __init__(self, n_job, n_machine, n_edge, batch, left_shift=True, obs_dtype="f64", device=0,
                 gamma=0.99, w_cfg=(0.4, 0.4, 0.2), scaling_divisor=1.0):
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceBatchEnv needs a GPU (MI355X); there is no CPU fallback")
        self.L = capi.lib()
        self.J, self.M, self.E, self.B = int(n_job), int(n_machine), int(n_edge), int(batch)
        self.T = self.J * self.M
        self.left_shift = bool(left_shift)
        self.gamma, self.w_cfg, self.scaling_divisor = float(gamma), tuple(float(x) for x in w_cfg), float(scaling_divisor)
        self.obs_f32 = obs_dtype in ("f32", torch.float32, np.float32)
        self.device = torch.device("cuda", device)
        cfg = capi.Config(self.J, self.M, self.E, self.B, int(bool(left_shift)), capi.OBS_F32 if self.obs_f32 else capi.OBS_F64,
                          device, 0, gamma, w_cfg[0], w_cfg[1], w_cfg[2], scaling_divisor)
        h = C.c_void_p()
        capi.check(self.L.mtfjsp_create(C.byref(cfg), C.byref(h)))
        self.h = h
        odt = torch.float32 if self.obs_f32 else torch.float64
        B, T, M, J = self.B, self.T, self.M, self.J
        dev = self.device
        # observation buffers are torch tensors so the rollout / PPO update can consume them zero-copy
        self.tasks_fea = torch.zeros(B * T, 12, dtype=odt, device=dev)
        self.ell_col = torch.full((B * T, 2), -1, dtype=torch.int32, device=dev)
        self.ell_val = torch.zeros(B * T, 2, dtype=torch.float32, device=dev)
        self.m_fea2 = torch.zeros(B, M, 8, dtype=odt, device=dev)
        self.info = torch.zeros(B, 6, dtype=torch.float64, device=dev)
        self.raw = torch.zeros(B, 5, dtype=torch.float64, device=dev)
        self.candidate = torch.zeros(B, J, dtype=torch.int32, device=dev)
        self.job_mask = torch.zeros(B, J, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.m_fea1 = torch.zeros(B, M, 6, dtype=odt, device=dev)
        self.mmask = torch.zeros(B, M, dtype=torch.uint8, device=dev)
        obs = capi.Obs(*[x.data_ptr() for x in (self.tasks_fea, self.ell_col, self.ell_val, self.m_fea2, self.info,
                                                  self.raw, self.candidate, self.job_mask, self.status)])
        capi.check(self.L.mtfjsp_bind_obs(self.h, C.byref(obs)), self.h)
        self._sp_buf = None
        self.use_current_stream()

    @classmethod
    def like(cls, src, batch):
        """a handle of `batch` instances like `src`: its sizes, left-shift setting, observation type, device, gamma, w_cfg and scaling divisor"""
        return cls(src.J, src.M, src.E, batch, left_shift=src.left_shift, obs_dtype="f32" if src.obs_f32 else "f64", device=src.device.index or 0,
                   gamma=src.gamma, w_cfg=src.w_cfg, scaling_divisor=src.scaling_divisor)

    def use_current_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.L.mtfjsp_set_stream(self.h, C.c_void_p(s)), self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.mtfjsp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- instances (= get_batch, pe:39-66)
    def load_instances(self, t, p, tt, edge=None, shop=None):
        t = np.ascontiguousarray(t, np.float64); p = np.ascontiguousarray(p, np.float64)
        tt = np.ascontiguousarray(tt, np.float64)
        assert t.shape == (self.B, self.T, self.M) and p.shape == t.shape and tt.shape == (self.B, self.M, self.M)
        shop = shop_of_machine(edge) if shop is None else np.ascontiguousarray(shop, np.int32)
        self._host_t = t
        capi.check(self.L.mtfjsp_load_instances_host(self.h, t.ctypes.data, p.ctypes.data, tt.ctypes.data, shop.ctypes.data), self.h)

    def load_instances_device(self, t, p, tt, shop):
        for x in (t, p, tt):
            assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
        assert shop.dtype == torch.int32
        capi.check(self.L.mtfjsp_load_instances(self.h, t.data_ptr(), p.data_ptr(), tt.data_ptr(), shop.data_ptr()), self.h)

    def generate_instances(self, seed, first_instance=0, scope=None):
        """draw this batch's instances ON the device: the distribution of the reference's Instance_Dataset
        (instances.DEFAULT_SCOPE = instance/config_ins.json), Philox keyed by (seed, first_instance + b); nothing is uploaded"""
        from .instances import DEFAULT_SCOPE
        sc = dict(DEFAULT_SCOPE)
        if scope:
            sc.update(scope)
        s9 = np.array([sc["t_low"], sc["t_high"], sc["p_low"], sc["p_high"], sc["weight_low"], sc["weight_high"],
                       sc["transT_in_low"], sc["transT_in_high"], sc["transT_out_high"]], np.float64)
        capi.check(self.L.mtfjsp_generate_instances(self.h, int(seed), int(first_instance), s9.ctypes.data), self.h)

    def read_instances(self):
        """-> (t, p [B,T,M], tt [B,M,M], edge [B,E,M/E]) host arrays of the loaded / generated instances"""
        B, T, M, E = self.B, self.T, self.M, self.E
        t = np.zeros((B, T, M)); p = np.zeros((B, T, M)); tt = np.zeros((B, M, M)); shop = np.zeros((B, M), np.int32)
        capi.check(self.L.mtfjsp_read_instances_host(self.h, t.ctypes.data, p.ctypes.data, tt.ctypes.data, shop.ctypes.data), self.h)
        edge = np.stack([np.stack([np.flatnonzero(shop[b] == e) for e in range(E)]) for b in range(B)]).astype(np.int64)
        return t, p, tt, edge

    # ---- fork (mtfjsp_fork: no reference counterpart; pdrs:465-540 replays the prefix instead)
    def fork_from(self, src, index, instance=True, state=True, obs=True):
        """instance i of this handle becomes a copy of instance index[i] of `src` (another DeviceBatchEnv of the same size, dtype,
        left-shift setting and device; any batch): one launch on this handle's stream, nothing is read back.  index: host sequence
        or int32 device tensor [B] (duplicates, any order; an entry outside [0, src.B) leaves that instance untouched and sets
        ST_INVALID in its status word).  instance / state / obs: the constants, the scheduling state (enough to step on), the bound
        observation (include/mtfjsp.h).  Both handles must be on one stream, or the caller orders them."""
        if not torch.is_tensor(index):
            index = torch.as_tensor(np.ascontiguousarray(index, np.int32), device=self.device)
        assert index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.shape == (self.B,)
        flags = (capi.FORK_INSTANCE if instance else 0) | (capi.FORK_STATE if state else 0) | (capi.FORK_OBS if obs else 0)
        self._fork_index = index                                        # alive until the launch has run
        capi.check(self.L.mtfjsp_fork(self.h, src.h, index.data_ptr(), flags), self.h)

    def state_signature(self, out=None):
        """64-bit order-independent signature of every instance's partial schedule (mtfjsp_state_signature: one launch, nothing read
        back) -> int64 device tensor [B] holding the unsigned words (`.cpu().numpy().view(np.uint64)`); 0 for a fresh instance"""
        if out is None:
            out = torch.empty(self.B, dtype=torch.int64, device=self.device)
        assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.shape == (self.B,)
        capi.check(self.L.mtfjsp_state_signature(self.h, out.data_ptr()), self.h)
        return out

    # ---- groups of copies (csrc/mtfjsp_group.hip): best-of-K evaluation on the fork
    def final_costs(self, out=None, done=None):
        """-> (cost4 [B,4] f64, done [B] uint8) device tensors: makespan, processing energy / T, transport time, idle time of every
        instance's schedule as it stands (`validate_cost_batched`'s Final_4cost, formed on the device) and whether all T
        operations are scheduled (mtfjsp_final_costs: one launch, nothing read back)"""
        if out is None:
            out = torch.empty(self.B, 4, dtype=torch.float64, device=self.device)
        if done is None:
            done = torch.empty(self.B, dtype=torch.uint8, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.shape == (self.B, 4)
        assert done.is_cuda and done.dtype == torch.uint8 and done.is_contiguous() and done.shape == (self.B,)
        capi.check(self.L.mtfjsp_final_costs(self.h, out.data_ptr(), done.data_ptr()), self.h)
        return out, done

    def replay_plans(self, task, mach, cost4=None, done=None, state=False):
        """The plans task, mach — int32 device tensors [T, stride >= B] in history layout (row s = the actions of step s, copy b = column
        b; a column-offset view of a wider buffer is fine: rows contiguous, one row stride) — replayed from scratch in ONE launch
        (mtfjsp_replay_plans): -> (cost4 [B,4] f64, done [B] uint8) device tensors, bit for bit what `reset`, T times `step` and
        `final_costs` give, except that a copy that is not done holds four NaNs.  The handle needs instances and no reset.
        state=True also writes every copy's schedule, so that `critical_path`, `state_signature` and `read_state` of STATE_MACHINE,
        _START, _FINISH, _ROUTES see it.  Until the next `reset` everything else that needs a state raises (MtfjspError, ERR_STATE):
        `step`, `final_costs`, a fork of state or observation out of this handle, the masks, the snapshots.  Nothing is read back."""
        T, B = self.T, self.B
        for x in (task, mach):
            assert x.is_cuda and x.dtype == torch.int32 and x.dim() == 2 and x.shape[0] == T and x.shape[1] >= B and x.stride(1) == 1
        assert T == 1 or task.stride(0) == mach.stride(0)
        stride = task.stride(0) if T > 1 else max(task.shape[1], B)
        if cost4 is None:
            cost4 = torch.empty(B, 4, dtype=torch.float64, device=self.device)
        if done is None:
            done = torch.empty(B, dtype=torch.uint8, device=self.device)
        assert cost4.is_cuda and cost4.dtype == torch.float64 and cost4.is_contiguous() and cost4.shape == (B, 4)
        assert done.is_cuda and done.dtype == torch.uint8 and done.is_contiguous() and done.shape == (B,)
        self._plan_keep = (task, mach)                                  # alive until the launch has run
        capi.check(self.L.mtfjsp_replay_plans(self.h, task.data_ptr(), mach.data_ptr(), stride, cost4.data_ptr(), done.data_ptr(),
                                              capi.REPLAY_STATE if state else 0), self.h)
        return cost4, done

    def group_reduce(self, N, K, cost4, done, w_cfg, obj=True, best=True, best_obj=True, front=True):
        """N groups of K copies (copy c of group n = element n*K + c of cost4 [N*K,4] f64 and done [N*K] uint8, device tensors
        from any source; this handle gives the device and the stream only).  w_cfg = (w_mk, w_ec, w_tt).  A copy is eligible iff
        done and none of its three objectives (makespan, energy + idle, transport) is NaN.
        -> (obj [N*K] f64: w_mk*mk + w_ec*ec + w_tt*tt in `validate_cost_batched`'s order, NaN where not eligible;
            best [N] int32: n*K + c of the eligible copy with the smallest obj, lowest c on ties, -1 without one;
            best_obj [N] f64: its obj, NaN without one;
            front [N*K] uint8: 1 iff eligible and not dominated inside its group, of exact duplicates the lowest c)
        device tensors; an output switched off (False) is None and is not computed.  An output may also be given as a tensor to
        write into.  1 <= K <= 4096.  One launch (mtfjsp_group_reduce), nothing read back."""
        N, K = int(N), int(K)
        assert cost4.is_cuda and cost4.dtype == torch.float64 and cost4.is_contiguous() and cost4.numel() == N * K * 4
        assert done.is_cuda and done.dtype == torch.uint8 and done.is_contiguous() and done.numel() == N * K
        dev = self.device
        # (an out-of-range N or K is the library's MTFJSP_ERR_ARG; the buffers below are then never written)
        obj = _out(obj, max(N * K, 0), torch.float64, dev); best = _out(best, max(N, 0), torch.int32, dev)
        best_obj = _out(best_obj, max(N, 0), torch.float64, dev); front = _out(front, max(N * K, 0), torch.uint8, dev)
        w = (C.c_double * 3)(*[float(x) for x in w_cfg])
        capi.check(self.L.mtfjsp_group_reduce(self.h, N, K, cost4.data_ptr(), done.data_ptr(), w, _ptr(obj), _ptr(best), _ptr(best_obj),
                                              _ptr(front)), self.h)
        return obj, best, best_obj, front

    # ---- neighbourhood moves on plans (csrc/mtfjsp_plan.hip): local search over the groups of copies
    def plan_neighbours(self, K, src_task, src_mach, src_col=None, seed=0, round=0, first_instance=0, moves=7, task_out=None, mach_out=None,
                        kind_out=True, critical=None):
        """This handle holds N groups of K copies (batch = N*K, copy c of group n = element n*K + c).  src_task, src_mach: int32
        device tensors [T, stride] in history layout (row s = the action of step s); the incumbent plan of group n is column
        src_col[n] (int32 device tensor [N], e.g. `best` of `group_reduce`) or column n without src_col.
        -> (task [T, N*K], mach [T, N*K], kind [N*K] int8) device tensors: copy 0 of every group is its incumbent (kind -1), every
        other copy the incumbent after one move drawn from `moves` (a mask of 1 SWAP, 2 INSERT, 4 REASSIGN; kind = the move drawn) by
        the Philox stream of (seed, first_instance + n, c, round) — include/mtfjsp.h has the rule.  Row s is ready for `step`.  A
        source column or an incumbent entry out of range gives a group of -1.  task_out / mach_out: tensors to write into (they must
        not overlap the sources); kind_out: True, a tensor, or None / False for no kinds.  One launch, nothing read back.
        critical = (path_task [N,T] int32, path_arc [N,T] int8, path_len [N] int32) as `critical_path` returns them for the incumbents'
        schedules: `moves` may then also hold 8 CRIT_SWAP (a machine arc of the path between two jobs is turned round) and 16
        CRIT_REASSIGN (a task of the path changes machine).  With `critical` or moves > 7 the call is
        mtfjsp_plan_neighbours_critical; with moves <= 7 both entries give the same words."""
        K, T, dev = int(K), self.T, self.device
        for x in (src_task, src_mach):
            assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and x.dim() == 2 and x.shape[0] == T
        assert src_mach.shape == src_task.shape
        if src_col is not None:
            assert src_col.is_cuda and src_col.dtype == torch.int32 and src_col.is_contiguous() and src_col.numel() * max(K, 1) == self.B
        task_out = torch.empty(T, self.B, dtype=torch.int32, device=dev) if task_out is None else task_out
        mach_out = torch.empty(T, self.B, dtype=torch.int32, device=dev) if mach_out is None else mach_out
        for x in (task_out, mach_out):
            assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and tuple(x.shape) == (T, self.B)
        kind_out = _out(kind_out, (self.B,), torch.int8, dev)
        self._plan_keep = (src_task, src_mach, src_col, critical)       # alive until the launch has run
        args = (self.h, K, src_task.data_ptr(), src_mach.data_ptr(), src_task.shape[1], _ptr(src_col), int(seed), int(round), int(first_instance),
                int(moves), task_out.data_ptr(), mach_out.data_ptr(), _ptr(kind_out))
        if critical is None and int(moves) <= 7:
            capi.check(self.L.mtfjsp_plan_neighbours(*args), self.h)
        else:
            path = (None, None, None) if critical is None else tuple(critical)
            if critical is not None:
                N = self.B // max(K, 1)
                for x, dt, shape in zip(path, (torch.int32, torch.int8, torch.int32), ((N, T), (N, T), (N,))):
                    assert x.is_cuda and x.dtype == dt and x.is_contiguous() and tuple(x.shape) == shape
            capi.check(self.L.mtfjsp_plan_neighbours_critical(*args, *(_ptr(x) for x in path)), self.h)
        return task_out, mach_out, kind_out

    def plan_offspring(self, P, src_task, src_mach, src_obj, src_best=None, seed=0, generation=0, first_instance=0, cross_thr=1 << 32,
                       mut_thr=0, moves=7, task_out=None, mach_out=None, parent_out=True, kind_out=True):
        """This handle holds N populations of P plans (batch = N*P, member c of group n = element n*P + c).  src_task, src_mach: int32
        device tensors [T, N*P] in history layout, the current population; src_obj [N*P] f64 and src_best [N] int32 (or None): `obj`
        and `best` of `group_reduce` for it.
        -> (task [T, N*P], mach [T, N*P], parent [N*P, 2] int32, kind [N*P] int8) device tensors, the offspring: with src_best child 0
        of every group is its best member word for word (parent -1, -1; kind -1); every other child has parents A and B chosen by two
        binary tournaments on src_obj, is crossed (precedence-preserving order crossover of the job strings, a coin per task for
        the machine) iff its Philox word is below cross_thr, takes one move of `plan_neighbours` out of `moves` iff another is below
        mut_thr (thresholds in [0, 2^32]), and is decoded.  parent = the columns of A and B (B = -1 without crossover); kind = 0
        without mutation, else the move drawn.  The draws are keyed by (seed, first_instance + n, c, generation) — include/mtfjsp.h
        has the rule.  A child that cannot be formed (a parent that is no plan) is a column of -1.  task_out / mach_out: tensors to
        write into (not overlapping the sources); parent_out / kind_out: True, a tensor, or None / False.  One launch
        (mtfjsp_plan_offspring), nothing read back."""
        P, T, B, dev = int(P), self.T, self.B, self.device
        for x in (src_task, src_mach):
            assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and tuple(x.shape) == (T, B)
        assert src_obj.is_cuda and src_obj.dtype == torch.float64 and src_obj.is_contiguous() and src_obj.numel() == B
        if src_best is not None:
            assert src_best.is_cuda and src_best.dtype == torch.int32 and src_best.is_contiguous() and src_best.numel() * max(P, 1) == B
        task_out = torch.empty(T, B, dtype=torch.int32, device=dev) if task_out is None else task_out
        mach_out = torch.empty(T, B, dtype=torch.int32, device=dev) if mach_out is None else mach_out
        for x in (task_out, mach_out):
            assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and tuple(x.shape) == (T, B)
        parent_out, kind_out = _out(parent_out, (B, 2), torch.int32, dev), _out(kind_out, (B,), torch.int8, dev)
        self._plan_keep = (src_task, src_mach, src_obj, src_best)       # alive until the launch has run
        capi.check(self.L.mtfjsp_plan_offspring(self.h, P, src_task.data_ptr(), src_mach.data_ptr(), src_obj.data_ptr(), _ptr(src_best), int(seed),
                                                int(generation), int(first_instance), int(cross_thr), int(mut_thr), int(moves),
                                                task_out.data_ptr(), mach_out.data_ptr(), _ptr(parent_out), _ptr(kind_out)), self.h)
        return task_out, mach_out, parent_out, kind_out

    # ---- multi-front selection (csrc/mtfjsp_nsga.hip): front ranks and survivors of parents and children together
    def front_rank(self, N, cost4_a, done_a, cost4_b=None, done_b=None, w_cfg=None, rank=True, crowd=True, order=True, front_size=True,
                   best_obj=True):
        """N groups of K = Ka + Kb candidates in two array sets (parents and children need no concatenation): candidate c < Ka of
        group n = element n*Ka + c of cost4_a [N*Ka,4] f64 and done_a [N*Ka] uint8, candidate c >= Ka = element n*Kb + (c - Ka) of
        cost4_b, done_b (None: Kb = 0).  Device tensors from any source; this handle gives the device and the stream only.  w_cfg =
        (w_mk, w_ec, w_tt), None: the handle's.  Objectives, eligibility and dominance are `group_reduce`'s.
        -> (rank [N*K] int32: the front index by peeling — rank 0 = `group_reduce`'s front, then the front of the rest, ...; -1 where
                not eligible;
            crowd [N*K] f64: the crowding distance inside the candidate's rank, +inf at the ends of an axis and for the member with
                the rank's smallest obj, NaN where not eligible;
            order [N*K] int32: the group's candidates in selection order (eligible first, ascending rank, descending crowd with NaN
                last, ascending index), order[n*K + i] = the local index c of the i-th;
            front_size [N] int32: the members of rank 0;  best_obj [N] f64: the smallest obj, NaN without an eligible candidate)
        device tensors — include/mtfjsp.h has the rule; an output switched off (False) is None and is not computed, an output may also
        be given as a tensor to write into.  1 <= K <= 2048.  One launch (mtfjsp_front_rank), nothing read back."""
        N, dev = int(N), self.device
        assert cost4_a.is_cuda and cost4_a.dtype == torch.float64 and cost4_a.is_contiguous() and N >= 1 and cost4_a.numel() % (4 * N) == 0
        Ka = cost4_a.numel() // (4 * N)
        assert done_a.is_cuda and done_a.dtype == torch.uint8 and done_a.is_contiguous() and done_a.numel() == N * Ka
        Kb = 0
        if cost4_b is not None:
            assert cost4_b.is_cuda and cost4_b.dtype == torch.float64 and cost4_b.is_contiguous() and cost4_b.numel() % (4 * N) == 0
            Kb = cost4_b.numel() // (4 * N)
            assert done_b is not None and done_b.is_cuda and done_b.dtype == torch.uint8 and done_b.is_contiguous() and done_b.numel() == N * Kb
        NK = N * (Ka + Kb)
        # (an out-of-range K is the library's MTFJSP_ERR_ARG; the buffers below are then never written)
        rank, crowd, order = _out(rank, NK, torch.int32, dev), _out(crowd, NK, torch.float64, dev), _out(order, NK, torch.int32, dev)
        front_size, best_obj = _out(front_size, N, torch.int32, dev), _out(best_obj, N, torch.float64, dev)
        w = (C.c_double * 3)(*[float(x) for x in (self.w_cfg if w_cfg is None else w_cfg)])
        capi.check(self.L.mtfjsp_front_rank(self.h, N, Ka, Kb, cost4_a.data_ptr(), done_a.data_ptr(), _ptr(cost4_b if Kb else None),
                                            _ptr(done_b if Kb else None), w, _ptr(rank), _ptr(crowd), _ptr(order), _ptr(front_size),
                                            _ptr(best_obj)), self.h)
        return rank, crowd, order, front_size, best_obj

    def plan_survivors(self, P, order, rank, a, b=None, task_out=None, mach_out=None, cost4_out=True, done_out=True, rank_out=True,
                       src_out=True, fit_out=True):
        """This handle holds N populations of P plans (batch = N*P).  a = (task [T, N*Ka], mach [T, N*Ka], cost4 [N*Ka,4], done [N*Ka]),
        b the same with Kb or None: the candidates `front_rank` ranked, plans in history layout; order, rank [N*K] int32: its
        outputs; 1 <= P <= K = Ka + Kb.  Column n*P + i of the outputs takes candidate c = order[n*K + i]:
        -> (task [T, N*P], mach [T, N*P] int32, cost4 [N*P,4] f64, done [N*P] uint8, rank [N*P] int32: the survivor's rank,
            src [N*P] int32: c, fit [N*P] f64: float(i) for an eligible survivor, NaN otherwise)
        device tensors.  The population is stored in selection order, so `plan_offspring` with src_obj = fit and no src_best runs
        the crowded tournaments of NSGA-II.  An order entry outside [0, K) gives a column of -1 with done 0.  task_out / mach_out:
        tensors to write into; the others True, a tensor, or None / False.  No output may overlap an input or another output.
        One launch (mtfjsp_plan_survivors), nothing read back."""
        P, T, B, dev = int(P), self.T, self.B, self.device
        assert P >= 1 and B % P == 0
        N = B // P
        K = []
        for s in (a, b):
            if s is None:
                K.append(0)
                continue
            tk, mc, c4, dn = s
            assert tk.is_cuda and tk.dtype == torch.int32 and tk.is_contiguous() and tk.dim() == 2 and tk.shape[0] == T and tk.shape[1] % N == 0
            k = tk.shape[1] // N
            assert mc.is_cuda and mc.dtype == torch.int32 and mc.is_contiguous() and mc.shape == tk.shape
            assert c4.is_cuda and c4.dtype == torch.float64 and c4.is_contiguous() and c4.numel() == N * k * 4
            assert dn.is_cuda and dn.dtype == torch.uint8 and dn.is_contiguous() and dn.numel() == N * k
            K.append(k)
        Ka, Kb = K
        for x in (order, rank):
            assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and x.numel() == N * (Ka + Kb)
        task_out = torch.empty(T, B, dtype=torch.int32, device=dev) if task_out is None else task_out
        mach_out = torch.empty(T, B, dtype=torch.int32, device=dev) if mach_out is None else mach_out
        for x in (task_out, mach_out):
            assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and tuple(x.shape) == (T, B)
        cost4_out, done_out = _out(cost4_out, (B, 4), torch.float64, dev), _out(done_out, (B,), torch.uint8, dev)
        rank_out, src_out, fit_out = _out(rank_out, (B,), torch.int32, dev), _out(src_out, (B,), torch.int32, dev), _out(fit_out, (B,), torch.float64, dev)
        self._plan_keep = (order, rank, a, b)                           # alive until the launch has run
        srcs = [_ptr(x) for x in a] + [_ptr(x) for x in (b if Kb else (None,) * 4)]
        capi.check(self.L.mtfjsp_plan_survivors(self.h, N, Ka, Kb, P, order.data_ptr(), rank.data_ptr(), *srcs, task_out.data_ptr(),
                                                mach_out.data_ptr(), _ptr(cost4_out), _ptr(done_out), _ptr(rank_out), _ptr(src_out),
                                                _ptr(fit_out)), self.h)
        return task_out, mach_out, cost4_out, done_out, rank_out, src_out, fit_out

    def critical_path(self, col=None, n=None, task_out=None, arc_out=None, len_out=None):
        """One critical path per row out of this handle's schedules as they stand (mtfjsp_critical_path: one launch, nothing read
        back).  col: int32 device tensor [n] — row i describes instance col[i]; an entry outside [0, B) gives an empty row — or None:
        row i = instance i, n = B.
        -> (path_task [n,T] int32, path_arc [n,T] int8, path_len [n] int32) device tensors: from the task that ends last backwards
        along tight arcs, the route predecessor first (arc 1), else the job predecessor (arc 0); -1 for the last element's arc and
        at and after path_len.  include/mtfjsp.h has the rule.  task_out / arc_out / len_out: tensors to write into."""
        dev, T = self.device, self.T
        if col is not None:
            assert col.is_cuda and col.dtype == torch.int32 and col.is_contiguous() and col.dim() == 1
            n = col.numel() if n is None else int(n)
            assert n <= col.numel()
        else:
            n = self.B if n is None else int(n)
        task_out = torch.empty(max(n, 0), T, dtype=torch.int32, device=dev) if task_out is None else task_out
        arc_out = torch.empty(max(n, 0), T, dtype=torch.int8, device=dev) if arc_out is None else arc_out
        len_out = torch.empty(max(n, 0), dtype=torch.int32, device=dev) if len_out is None else len_out
        for x, dt, shape in ((task_out, torch.int32, (n, T)), (arc_out, torch.int8, (n, T)), (len_out, torch.int32, (n,))):
            assert x.is_cuda and x.dtype == dt and x.is_contiguous() and tuple(x.shape) == shape
        self._crit_keep = col                                           # alive until the launch has run
        capi.check(self.L.mtfjsp_critical_path(self.h, n, _ptr(col), task_out.data_ptr(),
                                               arc_out.data_ptr(), len_out.data_ptr()), self.h)
        return task_out, arc_out, len_out

    # ---- a walk on plans (csrc/mtfjsp_walk.hip): acceptance with a tabu ring, a slack and a late ring in the local search's round
    def walk_state(self, N, late_len=0, tabu_len=0):
        """-> the state `walk_accept` keeps for N groups: dict(late [N,late_len] f64 or None, tabu [N,tabu_len] int64 (the unsigned words)
        or None, tabu_n [N] int32 or None, best_obj [N] f64, best_task, best_mach [T,N] int32), uninitialised device tensors: the first
        call (first=True) fills them"""
        N, L, U, dev = int(N), int(late_len), int(tabu_len), self.device
        return dict(late=torch.empty(N, L, dtype=torch.float64, device=dev) if L > 0 else None,
                    tabu=torch.empty(N, U, dtype=torch.int64, device=dev) if U > 0 else None,
                    tabu_n=torch.empty(N, dtype=torch.int32, device=dev) if U > 0 else None,
                    best_obj=torch.empty(N, dtype=torch.float64, device=dev),
                    best_task=torch.empty(self.T, N, dtype=torch.int32, device=dev), best_mach=torch.empty(self.T, N, dtype=torch.int32, device=dev))

    def walk_accept(self, N, K, cost4, done, w_cfg, task, mach, state, sig=None, round=0, first=False, slack=None, next_col=None,
                    cur_obj=True, best_obj=True, pick=True, why=True, barred=True, obj=True):
        """N groups of K copies (copy c of group n = element n*K + c; copy 0 the incumbent) after the replay of the plans task, mach
        [T, N*K] int32: cost4 [N*K,4] f64 and done [N*K] uint8 as `final_costs` gives them, sig [N*K] int64 as `state_signature` gives
        it (or None), w_cfg = (w_mk, w_ec, w_tt).  This handle gives T, the device and the stream only.  state: the dict of
        `walk_state` — its shapes give late_len and tabu_len; first=True fills it.  The rule (include/mtfjsp.h): the candidates are the
        copies c >= 1 with an objective whose schedule is neither the incumbent's nor in the tabu ring; the best of them (lowest c
        among equals) is taken if strictly better (why 2), else if within `slack` of the incumbent (why 3; None: off, 0.0: sideways
        steps, inf: always), else if not above the late ring's entry of this round (why 4), else refused (why 1; 0: no candidate); a
        move into a new best adds 8 and stores the plan in state.
        -> (next_col [N] int32: the next incumbent's column, for `plan_neighbours`' src_col; cur_obj [N] f64: its objective; best_obj
            [N] f64: the best so far; pick [N] int32: the local index taken or refused, -1 without one; why [N] int8; barred [N] int32:
            candidates the two schedule tests removed; obj [N*K] f64 as `group_reduce` gives it)
        device tensors; next_col may be a tensor to write into; the others True, a tensor, or None / False.  A tabu ring needs sig.
        One launch (mtfjsp_walk_accept), nothing read back."""
        N, K, T, dev = int(N), int(K), self.T, self.device
        assert cost4.is_cuda and cost4.dtype == torch.float64 and cost4.is_contiguous() and cost4.numel() == N * K * 4
        assert done.is_cuda and done.dtype == torch.uint8 and done.is_contiguous() and done.numel() == N * K
        assert sig is None or (sig.is_cuda and sig.dtype == torch.int64 and sig.is_contiguous() and sig.numel() == N * K)
        for x in (task, mach):
            assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and tuple(x.shape) == (T, N * K)
        late, tabu, tabu_n = state["late"], state["tabu"], state["tabu_n"]
        late_len, tabu_len = (0 if late is None else late.shape[1]), (0 if tabu is None else tabu.shape[1])
        for x, dt, shape in ((late, torch.float64, (N, late_len)), (tabu, torch.int64, (N, tabu_len)), (tabu_n, torch.int32, (N,)),
                             (state["best_obj"], torch.float64, (N,)), (state["best_task"], torch.int32, (T, N)), (state["best_mach"], torch.int32, (T, N))):
            assert x is None or (x.is_cuda and x.dtype == dt and x.is_contiguous() and tuple(x.shape) == shape)
        assert (tabu is None) == (tabu_n is None)
        # (an out-of-range N or K is the library's MTFJSP_ERR_ARG; the buffers below are then never written)
        next_col = _out(True if next_col is None else next_col, max(N, 0), torch.int32, dev)
        cur_obj, best_obj = _out(cur_obj, max(N, 0), torch.float64, dev), _out(best_obj, max(N, 0), torch.float64, dev)
        pick, why, barred = _out(pick, max(N, 0), torch.int32, dev), _out(why, max(N, 0), torch.int8, dev), _out(barred, max(N, 0), torch.int32, dev)
        obj = _out(obj, max(N * K, 0), torch.float64, dev)
        w = (C.c_double * 3)(*[float(x) for x in w_cfg])
        self._plan_keep = (cost4, done, sig, task, mach, state)         # alive until the launch has run
        capi.check(self.L.mtfjsp_walk_accept(self.h, N, K, cost4.data_ptr(), done.data_ptr(), w, _ptr(sig), task.data_ptr(), mach.data_ptr(),
                                             int(round), int(bool(first)), -1.0 if slack is None else float(slack), late_len, tabu_len,
                                             _ptr(late), _ptr(tabu), _ptr(tabu_n), state["best_obj"].data_ptr(), state["best_task"].data_ptr(),
                                             state["best_mach"].data_ptr(), next_col.data_ptr(), _ptr(cur_obj), _ptr(best_obj), _ptr(pick),
                                             _ptr(why), _ptr(barred), _ptr(obj)), self.h)
        return next_col, cur_obj, best_obj, pick, why, barred, obj

    def scaler_init(self):
        capi.check(self.L.mtfjsp_scaler_init(self.h), self.h)

    def scaler_reset_returns(self):
        capi.check(self.L.mtfjsp_scaler_reset_returns(self.h), self.h)

    def scaler_reset_returns_masked(self, mask):
        m = np.ascontiguousarray(mask, np.uint8)
        assert m.shape == (self.B,)
        capi.check(self.L.mtfjsp_scaler_reset_returns_masked_host(self.h, m.ctypes.data), self.h)

    # ---- reset / step
    def reset(self, w3):
        if torch.is_tensor(w3):
            assert w3.is_cuda and w3.dtype == torch.float64 and w3.is_contiguous()
            self._w3 = w3
            capi.check(self.L.mtfjsp_reset(self.h, w3.data_ptr()), self.h)
        else:
            w3 = np.ascontiguousarray(w3, np.float64)
            assert w3.shape == (self.B, 3)
            capi.check(self.L.mtfjsp_reset_host(self.h, w3.ctypes.data), self.h)

    def reset_episode(self, seed, episode, out=None, reset_returns=True):
        """scaler_reset_returns() + draw_reward_weights(seed, episode) + reset(those weights) in ONE launch -> the weights [B,3] f64"""
        if out is None:
            out = torch.empty(self.B, 3, dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
        self._w3 = out
        capi.check(self.L.mtfjsp_reset_episode(self.h, int(seed), int(episode), out.data_ptr(), 1 if reset_returns else 0), self.h)
        return out

    def draw_reward_weights(self, seed, episode, out=None):
        """reward weights of one episode drawn on the device (env:1253-1259 type "01", Philox keyed by (seed, episode, b)) -> [B,3] f64"""
        if out is None:
            out = torch.empty(self.B, 3, dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
        capi.check(self.L.mtfjsp_draw_reward_weights(self.h, int(seed), int(episode), out.data_ptr()), self.h)
        return out

    def step(self, task_idx, mach_idx):
        """device tensors (int32) -> asynchronous launch; numpy/list -> host variant (raises on invalid actions)."""
        if torch.is_tensor(task_idx):
            assert task_idx.is_cuda and task_idx.dtype == torch.int32 and mach_idx.dtype == torch.int32
            capi.check(self.L.mtfjsp_step(self.h, task_idx.data_ptr(), mach_idx.data_ptr()), self.h)
        else:
            a = np.ascontiguousarray(task_idx, np.int32); m = np.ascontiguousarray(mach_idx, np.int32)
            assert a.shape == (self.B,) and m.shape == (self.B,)
            capi.check(self.L.mtfjsp_step_host(self.h, a.ctypes.data, m.ctypes.data), self.h)

    def step_record(self, task_idx, mach_idx, r4_out, done_out):
        """device step that also writes this step's f32 trajectory entries: r4_out [4,B], done_out [B] (contiguous views)"""
        assert r4_out.is_contiguous() and done_out.is_contiguous() and r4_out.dtype == torch.float32
        capi.check(self.L.mtfjsp_step_record(self.h, task_idx.data_ptr(), mach_idx.data_ptr(), r4_out.data_ptr(), done_out.data_ptr()), self.h)

    def step_kernel_name(self):
        """the step kernel the next step() launches (shape, this device's LDS, the diagnostic switches as they are now)"""
        return self.L.mtfjsp_step_kernel_name(self.h).decode()

    def step_launch_info(self):
        """(instances per workgroup, dynamic LDS bytes, LDS bytes a workgroup may use on this device) of the launch step_kernel_name names"""
        g, nb, mx = C.c_int32(), C.c_int64(), C.c_int64()
        capi.check(self.L.mtfjsp_step_launch_info(self.h, C.byref(g), C.byref(nb), C.byref(mx)), self.h)
        return g.value, nb.value, mx.value

    def step_params(self, task_idx, mach_idx, r4_out=None, done_out=None):
        """the parameter block of exactly the step that step() / step_record() with these arguments would launch, for
        Encoder.arm_env_step (the step then rides in the machine actor's heads launch) — or None when this environment's step
        cannot (shape, kernel-time recording, diagnostic overrides): then call step() / step_record() as usual"""
        if self._sp_buf is None:
            self._sp_buf = C.create_string_buffer(int(self.L.mtfjsp_step_params_bytes()))
        rc = self.L.mtfjsp_step_params(self.h, task_idx.data_ptr(), mach_idx.data_ptr(), r4_out.data_ptr() if r4_out is not None else None,
                                       done_out.data_ptr() if done_out is not None else None, self._sp_buf, len(self._sp_buf))
        if rc < 0:
            capi.check(rc, self.h)
        return self._sp_buf if rc == 1 else None

    def gae(self, r, v, v_next, done, gamma, lam, out=None):
        """un-normalised GAE advantages [S,B] for one reward channel.  Only r / v / v_next may be strided views (arbitrary (s,b)
        element strides); done and out must be contiguous [S,B] — out may be a contiguous slice of a larger packed buffer"""
        S = done.shape[0]
        if out is None:
            out = torch.empty(S, self.B, dtype=torch.float32, device=self.device)
        assert done.is_contiguous() and out.is_contiguous()
        capi.check(self.L.mtfjsp_gae(self.h, S, r.data_ptr(), r.stride(0), r.stride(1), v.data_ptr(), v.stride(0), v.stride(1),
                                     v_next.data_ptr(), v_next.stride(0), v_next.stride(1), done.data_ptr(), gamma, lam, out.data_ptr()), self.h)
        return out

    @staticmethod
    def _view_table(views):
        """K f32 [S,B] views (any element strides) -> (pointer array, stride_s array, stride_b array) for the C ABI"""
        K = len(views)
        ptrs = (C.c_void_p * K)(*[(v.data_ptr() if v is not None else None) for v in views])
        ss = (C.c_int64 * K)(*[(v.stride(0) if v is not None else 0) for v in views])
        sb = (C.c_int64 * K)(*[(v.stride(1) if v is not None else 0) for v in views])
        return ptrs, ss, sb

    def pack_views(self, views, out):
        """K strided f32 [S,B] views -> out[k] (out: contiguous [K,S,B] or a contiguous slice of a larger packed buffer); one launch"""
        K, S = len(views), views[0].shape[0]
        assert out.is_contiguous() and tuple(out.shape) == (K, S, self.B) and all(v.dtype == torch.float32 for v in views)
        ptrs, ss, sb = self._view_table(views)
        capi.check(self.L.mtfjsp_pack_views(self.h, K, S, ptrs, ss, sb, out.data_ptr()), self.h)
        return out

    def normalize_advantages(self, gathered, K, world, rank, values, norm_out, targets_out=None, full_out=None, eps=1e-5):
        """(adv - mean) / (std + eps) of ppo:485,532 for the first K tensors of gathered [world, K_total, S, B] (statistics over all
        shards' columns), value targets = normalised advantage + values[k] ([S,B] views), optional reference layout
        full_out [K_total, S, world*B]; two launches, no torch kernels (include/mtfjsp.h)"""
        Kt, S = gathered.shape[-3], gathered.shape[-2]
        assert gathered.is_contiguous() and gathered.dtype == torch.float32 and gathered.numel() == world * Kt * S * self.B
        assert norm_out.is_contiguous() and (targets_out is None or targets_out.is_contiguous()) and (full_out is None or full_out.is_contiguous())
        ptrs = ss = sb = None
        if targets_out is not None:
            ptrs, ss, sb = self._view_table(list(values) + [None] * (K - len(values)))
        capi.check(self.L.mtfjsp_normalize_advantages(self.h, K, Kt, world, rank, S, gathered.data_ptr(), eps, ptrs, ss, sb, norm_out.data_ptr(),
                                                      targets_out.data_ptr() if targets_out is not None else None,
                                                      full_out.data_ptr() if full_out is not None else None), self.h)

    def observe_mfea1(self, task_idx, mmask=None):
        if not torch.is_tensor(task_idx):
            task_idx = torch.as_tensor(np.ascontiguousarray(task_idx, np.int32), device=self.device)
        mm = 0
        if mmask is not None:
            if not torch.is_tensor(mmask):
                mmask = torch.as_tensor(np.ascontiguousarray(np.asarray(mmask).reshape(self.B, self.M), np.uint8), device=self.device)
            mm = mmask.data_ptr()
        self._keep = (task_idx, mmask)
        capi.check(self.L.mtfjsp_observe_mfea1(self.h, task_idx.data_ptr(), mm, self.m_fea1.data_ptr(), self.mmask.data_ptr()), self.h)
        return self.m_fea1

    def observe_mfea1_jobs(self, out=None, mmask_out=None):
        """m_fea1 and the machine mask of EVERY job's candidate task (mtfjsp_observe_mfea1_jobs: one launch, nothing read back):
        row (b, j) is what `observe_mfea1` writes for task_idx[b] = candidate[b][j].  -> (out [B,J,M,6] observation dtype,
        mmask_out [B,J,M] uint8) device tensors; either may be given to write into"""
        B, J, M = self.B, self.J, self.M
        out = _out(True if out is None else out, (B, J, M, 6), torch.float32 if self.obs_f32 else torch.float64, self.device)
        mmask_out = _out(True if mmask_out is None else mmask_out, (B, J, M), torch.uint8, self.device)
        capi.check(self.L.mtfjsp_observe_mfea1_jobs(self.h, out.data_ptr(), mmask_out.data_ptr()), self.h)
        return out, mmask_out

    def mfea1_context(self):
        """device-pointer recipe of observe_mfea1 (-> self.m_fea1, self.mmask) for the encoder's heads kernel to execute right
        after it has selected the task (capi.Mfea1Ctx; valid while the instances stay loaded)"""
        ctx = capi.Mfea1Ctx()
        capi.check(self.L.mtfjsp_get_mfea1_context(self.h, self.m_fea1.data_ptr(), self.mmask.data_ptr(), C.byref(ctx)), self.h)
        return ctx

    def random_actions(self, seed, counter, task_idx, mach_idx, job_idx=None):
        capi.check(self.L.mtfjsp_random_actions(self.h, seed, counter, task_idx.data_ptr(), mach_idx.data_ptr(),
                                                job_idx.data_ptr() if job_idx is not None else 0), self.h)

    # ---- exports
    def dense_adj(self):
        out = torch.empty(self.B, self.T, self.T, dtype=torch.float64, device=self.device)
        capi.check(self.L.mtfjsp_export_dense_adj(self.h, out.data_ptr()), self.h)
        return out

    def valid_action_mask(self):
        out = torch.empty(self.B, self.T, dtype=torch.uint8, device=self.device)
        capi.check(self.L.mtfjsp_valid_action_mask(self.h, out.data_ptr()), self.h)
        return out

    def set_scaler_state(self, first, state17):
        """restore the RewardScaling state ([n,17], MTFJSP_STATE_SCALER layout) of instances first..first+n-1"""
        a = np.ascontiguousarray(state17, np.float64).reshape(-1, 17)
        capi.check(self.L.mtfjsp_set_scaler_state_host(self.h, int(first), a.shape[0], a.ctypes.data), self.h)

    def read_state(self, which):
        B, T, M = self.B, self.T, self.M
        shape, dt = {capi.STATE_MACHINE: ((B, T), np.int32), capi.STATE_START: ((B, T), np.float64),
                     capi.STATE_FINISH: ((B, T), np.float64), capi.STATE_ROUTES: ((B, M, T), np.int32),
                     capi.STATE_PREV_COSTS: ((B, 4), np.float64), capi.STATE_SCALER: ((B, 17), np.float64),
                     capi.STATE_W3: ((B, 3), np.float64)}[which]
        out = np.zeros(shape, dt)
        capi.check(self.L.mtfjsp_read_state_host(self.h, which, out.ctypes.data), self.h)
        return out

    def synchronize(self):
        capi.check(self.L.mtfjsp_synchronize(self.h), self.h)

    def footprint_copy(self, read_bytes, write_bytes, access_bytes=16, grid=2048, reps=50):
        """measurement only: (average, minimum) microseconds per launch of a plain streaming kernel with this footprint"""
        a, m = C.c_double(), C.c_double()
        capi.check(self.L.mtfjsp_footprint_copy(self.h, int(read_bytes), int(write_bytes), int(access_bytes), int(grid), int(reps),
                                                C.byref(a), C.byref(m)), self.h)
        return a.value, m.value

    def timing_begin(self):
        capi.check(self.L.mtfjsp_timing_begin(self.h), self.h)

    def timing_end(self):
        ms = C.c_double(); n = C.c_int64()
        capi.check(self.L.mtfjsp_timing_end(self.h, C.byref(ms), C.byref(n)), self.h)
        return ms.value, n.value
