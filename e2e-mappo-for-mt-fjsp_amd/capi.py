"""ctypes binding of include/mtfjsp.h (thin: no logic, only prototypes).

Fails loudly when libmtfjsp.so is missing — there is no CPU fallback for the product path.
"""
import ctypes as C
import os

from . import _build

_LIB = None

OBS_F64, OBS_F32 = 0, 1
OK, ERR_ARG, ERR_STATE, ERR_HIP, ERR_ACTION, ERR_RETRY = 0, -1, -2, -3, -4, -5
PATH_MASK, ST_INVALID, ST_INFEASIBLE = 0x7, 0x100, 0x200
FORK_INSTANCE, FORK_STATE, FORK_OBS = 1, 2, 4
REPLAY_STATE = 1
STATE_MACHINE, STATE_START, STATE_FINISH, STATE_ROUTES, STATE_PREV_COSTS, STATE_SCALER, STATE_W3 = range(7)


class Config(C.Structure):
    _fields_ = [("n_job", C.c_int32), ("n_machine", C.c_int32), ("n_edge", C.c_int32), ("batch", C.c_int32),
                ("left_shift", C.c_int32), ("obs_dtype", C.c_int32), ("device_id", C.c_int32), ("reserved", C.c_int32),
                ("gamma", C.c_double), ("w_mk", C.c_double), ("w_ec", C.c_double), ("w_tt", C.c_double),
                ("scaling_divisor", C.c_double)]


class Obs(C.Structure):
    _fields_ = [("tasks_fea", C.c_void_p), ("ell_col", C.c_void_p), ("ell_val", C.c_void_p), ("m_fea2", C.c_void_p),
                ("info", C.c_void_p), ("raw", C.c_void_p), ("candidate", C.c_void_p), ("job_mask", C.c_void_p),
                ("status", C.c_void_p)]


class Mfea1Ctx(C.Structure):
    _fields_ = [("t", C.c_void_p), ("p", C.c_void_p), ("tt", C.c_void_p), ("mean3", C.c_void_p), ("shop", C.c_void_p),
                ("link", C.c_void_p), ("m_fea1_out", C.c_void_p), ("mmask_out", C.c_void_p),
                ("T", C.c_int32), ("M", C.c_int32), ("obs_f32", C.c_int32), ("m_fea2", C.c_void_p)]


class EncoderConfig(C.Structure):
    _fields_ = [("n_job", C.c_int32), ("n_machine", C.c_int32), ("batch", C.c_int32), ("hidden", C.c_int32),
                ("obs_dtype", C.c_int32), ("device_id", C.c_int32)]


_VP, _I, _U64, _SZ = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t
PROTOTYPES = {
    # name: (restype, argtypes)
    "mtfjsp_create": (_I, [C.POINTER(Config), C.POINTER(_VP)]),
    "mtfjsp_destroy": (_I, [_VP]),
    "mtfjsp_last_error": (C.c_char_p, [_VP]),
    "mtfjsp_set_stream": (_I, [_VP, _VP]),
    "mtfjsp_synchronize": (_I, [_VP]),
    "mtfjsp_alloc_obs": (_I, [_VP, C.POINTER(Obs)]),
    "mtfjsp_bind_obs": (_I, [_VP, C.POINTER(Obs)]),
    "mtfjsp_snapshot_obs": (_I, [_VP, C.POINTER(Obs)]),
    "mtfjsp_snapshot_obs2": (_I, [_VP, C.POINTER(Obs), C.POINTER(Obs), _VP]),
    "mtfjsp_generate_instances": (_I, [_VP, _U64, _U64, _VP]),
    "mtfjsp_read_instances_host": (_I, [_VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_load_instances": (_I, [_VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_load_instances_host": (_I, [_VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_scaler_init": (_I, [_VP]),
    "mtfjsp_scaler_reset_returns": (_I, [_VP]),
    "mtfjsp_scaler_reset_returns_masked_host": (_I, [_VP, _VP]),
    "mtfjsp_reset": (_I, [_VP, _VP]),
    "mtfjsp_draw_reward_weights": (_I, [_VP, _U64, _U64, _VP]),
    "mtfjsp_reset_episode": (_I, [_VP, _U64, _U64, _VP, C.c_int32]),
    "mtfjsp_reset_host": (_I, [_VP, _VP]),
    "mtfjsp_step": (_I, [_VP, _VP, _VP]),
    "mtfjsp_step_host": (_I, [_VP, _VP, _VP]),
    "mtfjsp_step_record": (_I, [_VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_step_params_bytes": (C.c_int32, []),
    "mtfjsp_step_params": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int32]),
    "mtfjsp_step_kernel_name": (C.c_char_p, [_VP]),
    "mtfjsp_step_launch_info": (_I, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mtfjsp_step_kernel_name_for": (C.c_char_p, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "mtfjsp_gae": (_I, [_VP, C.c_int32, _VP, C.c_int64, C.c_int64, _VP, C.c_int64, C.c_int64, _VP, C.c_int64, C.c_int64, _VP, C.c_float, C.c_float, _VP]),
    "mtfjsp_normalize_advantages": (_I, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, C.c_float, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_pack_views": (_I, [_VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP]),
    "mtfjsp_observe_mfea1": (_I, [_VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_random_actions": (_I, [_VP, _U64, _U64, _VP, _VP, _VP]),
    "mtfjsp_pdr_plan": (_I, [_VP, _VP, _VP, _VP, _U64, _VP, _VP]),
    "mtfjsp_fork": (_I, [_VP, _VP, _VP, C.c_int32]),
    "mtfjsp_lookahead_expand": (_I, [_VP, _VP, _VP, _VP]),
    "mtfjsp_lookahead_select": (_I, [_VP, _VP, C.c_int32, _VP, _VP, _VP, _VP]),
    "mtfjsp_state_signature": (_I, [_VP, _VP]),
    "mtfjsp_beam_select": (_I, [_VP, _VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_beam_backtrack": (_I, [_VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_observe_mfea1_jobs": (_I, [_VP, _VP, _VP]),
    "mtfjsp_beam_select_policy": (_I, [_VP, C.c_int32] + [_VP] * 11),
    "mtfjsp_beam_merge_slots": (_I, [_VP, C.c_int32, _VP, _VP]),
    "mtfjsp_final_costs": (_I, [_VP, _VP, _VP]),
    "mtfjsp_group_reduce": (_I, [_VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_replay_plans": (_I, [_VP, _VP, _VP, C.c_int64, _VP, _VP, C.c_int32]),
    "mtfjsp_replay_launch_info_for": (_I, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "mtfjsp_plan_neighbours": (_I, [_VP, C.c_int32, _VP, _VP, C.c_int64, _VP, _U64, _U64, _U64, C.c_uint32, _VP, _VP, _VP]),
    "mtfjsp_plan_neighbours_critical": (_I, [_VP, C.c_int32, _VP, _VP, C.c_int64, _VP, _U64, _U64, _U64, C.c_uint32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mtfjsp_critical_path": (_I, [_VP, C.c_int32, _VP, _VP, _VP, _VP]),
    "mtfjsp_walk_accept": (_I, [_VP, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _U64, C.c_int32, C.c_double, C.c_int32, C.c_int32]
                           + [_VP] * 13),
    "mtfjsp_plan_offspring": (_I, [_VP, C.c_int32, _VP, _VP, _VP, _VP, _U64, _U64, _U64, _U64, _U64, C.c_uint32, _VP, _VP, _VP, _VP]),
    "mtfjsp_front_rank": (_I, [_VP, C.c_int32, C.c_int32, C.c_int32] + [_VP] * 10),
    "mtfjsp_plan_survivors": (_I, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_VP] * 17),
    "mtfjsp_export_dense_adj": (_I, [_VP, _VP]),
    "mtfjsp_export_dense_adj_host": (_I, [_VP, _VP]),
    "mtfjsp_valid_action_mask": (_I, [_VP, _VP]),
    "mtfjsp_read_state_host": (_I, [_VP, _I, _VP]),
    "mtfjsp_set_scaler_state_host": (_I, [_VP, _I, _I, _VP]),
    "mtfjsp_copy_to_host": (_I, [_VP, _VP, _VP, _SZ]),
    "mtfjsp_footprint_copy": (_I, [_VP, _SZ, _SZ, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mtfjsp_timing_begin": (_I, [_VP]),
    "mtfjsp_timing_end": (_I, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mtfjsp_encoder_create": (_I, [C.POINTER(EncoderConfig), C.POINTER(_VP)]),
    "mtfjsp_encoder_destroy": (_I, [_VP]),
    "mtfjsp_encoder_last_error": (C.c_char_p, [_VP]),
    "mtfjsp_encoder_set_stream": (_I, [_VP, _VP]),
    "mtfjsp_encoder_load_weight_host": (_I, [_VP, C.c_char_p, _VP, C.c_int64]),
    "mtfjsp_encoder_weights_ready": (_I, [_VP]),
    "mtfjsp_job_actor_forward": (_I, [_VP] * 11),
    "mtfjsp_machine_actor_forward": (_I, [_VP] * 8),
    "mtfjsp_global_critic_forward": (_I, [_VP] * 7),
    "mtfjsp_sample_categorical": (_I, [_VP, _VP, C.c_int32, C.c_int32, _U64, _U64, _VP, _VP, _VP, _VP]),
    "mtfjsp_encoder_set_bn_mode": (_I, [_VP, C.c_int32]),
    "mtfjsp_encoder_set_product_mode": (_I, [_VP, C.c_int32]),
    "mtfjsp_encoder_set_stats_reduce": (_I, [_VP, C.c_void_p, _VP, C.c_int64]),
    "mtfjsp_encoder_set_deferred_poll": (_I, [_VP, C.c_int32]),
    "mtfjsp_get_mfea1_context": (_I, [_VP, _VP, _VP, C.POINTER(Mfea1Ctx)]),
    "mtfjsp_encoder_arm_mfea1": (_I, [_VP, C.POINTER(Mfea1Ctx)]),
    "mtfjsp_encoder_arm_machine_heads": (_I, [_VP, _VP, _VP, _VP]),
    "mtfjsp_encoder_fused_launches": (_I, [_VP, C.POINTER(C.c_int64)]),
    "mtfjsp_encoder_arm_env_step": (_I, [_VP, _VP, C.c_int32]),
    "mtfjsp_encoder_arm_values_only": (_I, [_VP]),
    "mtfjsp_encoder_env_step_fused": (_I, [_VP]),
    "mtfjsp_encoder_arm_selection": (_I, [_VP, C.c_int32, C.c_int32, _U64, _U64, _VP, _VP, _VP, _VP]),
    "mtfjsp_hostgen_infeasible": (_I, [_VP, C.POINTER(C.c_int32), C.c_int64, _I, _I, C.c_int64, C.c_int64, _VP]),
    "mtfjsp_hostgen_transport": (_I, [_VP, C.POINTER(C.c_int32), C.c_int64, _I, _VP, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int64, _VP]),
    "mtfjsp_encoder_check": (_I, [_VP, C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_resident_failures": (_I, [_VP, C.POINTER(C.c_int64)]),
    "mtfjsp_gin_res_kernel_name_for": (C.c_char_p, [C.c_int32] * 6 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_gin_res_kernel_name": (C.c_char_p, [_VP]),
    "mtfjsp_gin_launches_for": (C.c_int32, [C.c_int32] * 6 + [C.c_uint32, C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_gin_launches": (C.c_int32, [_VP, C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_peek_gin_res_host": (_I, [_VP, _VP, C.c_int64, _VP, _VP]),
    "mtfjsp_fused3_kernel_name_for": (C.c_char_p, [C.c_int32] * 6 + [C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_fused3_kernel_name": (C.c_char_p, [_VP]),
    "mtfjsp_heads_kernel_name_for": (C.c_char_p, [C.c_int32] * 5 + [C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_heads_kernel_name": (C.c_char_p, [_VP, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_peek_fused3_host": (_I, [_VP, _VP, _VP]),
    "mtfjsp_encoder_range_fallbacks": (_I, [_VP, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "mtfjsp_encoder_peek_nodes_host": (_I, [_VP, _VP, C.c_int64]),
    "mtfjsp_encoder_device_allocations": (_I, [_VP, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mtfjsp_encoder_timing_begin": (_I, [_VP]),
    "mtfjsp_encoder_timing_end": (_I, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mtfjsp_encoder_timing_query": (_I, [_VP, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}


def lib_path():
    return os.environ.get("MTFJSP_LIB") or _build.LIB          # MTFJSP_LIB: diagnostic builds only (tools/)


def lib():
    """Load libmtfjsp.so.  Raises if it has not been built: the product never falls back to CPU."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build the HIP extension first (python __graft_entry__.py build, "
                "or python e2e-mappo-for-mt-fjsp_amd/_build.py). There is no CPU fallback.")
        L = C.CDLL(path)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)          # AttributeError if the library does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        _LIB = L
    return _LIB


class MtfjspError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmtfjsp error {code}: {msg}")
        self.code = code


def check(rc, handle=None, enc=False):
    if rc != 0:
        L = lib()
        msg = (L.mtfjsp_encoder_last_error(handle) if enc else L.mtfjsp_last_error(handle)) or b""
        raise MtfjspError(rc, msg.decode())


def replay_launch_info_for(n_job, n_machine, batch, lds_max=160 * 1024):
    """(copies per workgroup, dynamic LDS bytes) of the launch `DeviceBatchEnv.replay_plans` makes for a handle of this shape where a
    workgroup may use `lds_max` bytes of LDS (gfx950: 160 KiB) — the library's own rule (csrc/mtfjsp_replay.hip), no GPU needed.
    ValueError for a shape mtfjsp_create refuses or whose single copy does not fit `lds_max`."""
    g, nb = C.c_int32(0), C.c_int64(0)
    if lib().mtfjsp_replay_launch_info_for(n_job, n_machine, batch, lds_max, C.byref(g), C.byref(nb)) != OK:
        raise ValueError(f"no plan replay in one launch for J{n_job}M{n_machine} B={batch} with {lds_max} bytes of LDS per workgroup")
    return g.value, nb.value


def gin_res_kernel_for(batch, n_job, n_machine, num_cu=256, candidates=None, node_output=False):
    """(kernel name or None, instances per workgroup, workgroups): which instantiation of the single-launch GIN kernel serves a forward of this
    shape — the library's own rule (csrc/mtfjsp_gin_res_select.h), no GPU needed.  candidates: per instance (default n_job, the job actor; 0: the
    global critic).  MTFJSP_GIN_RES_GENERIC=1 in the environment forces the run-time kernel."""
    ipc, grid = C.c_int32(0), C.c_int32(0)
    name = lib().mtfjsp_gin_res_kernel_name_for(batch, n_job * n_machine, n_job, n_job if candidates is None else candidates, num_cu,
                                                int(bool(node_output)), C.byref(ipc), C.byref(grid))
    return (name.decode() if name else None), ipc.value, grid.value


# flag bits of mtfjsp_gin_launches_for (include/mtfjsp.h)
GIN_CRITIC, GIN_NODE_OUTPUT, GIN_PER_INSTANCE, GIN_OBS_F64, GIN_NO_SINGLE, GIN_REDUCE = 1, 2, 4, 8, 16, 32


def _gin_launches(call):
    """{path, pool, steps: [(family, kernel, rev, nt, reduce)], rpr, pool_grid} from one of the two report entries"""
    buf, order, pool = C.create_string_buffer(1024), (C.c_int32 * 12)(), (C.c_int32 * 2)()
    n = call(buf, len(buf), order, pool)
    if n < 0:
        return None
    path, form, seq = buf.value.decode().split(";")
    steps = [tuple(s.split(":")) + (order[i] & 1, order[i] >> 1 & 1, order[i] >> 2) for i, s in enumerate(seq.split(","))]
    assert len(steps) == n
    return {"path": path, "pool": form, "steps": steps, "rpr": pool[0], "pool_grid": pool[1]}


def gin_launches_for(batch, n_job, n_machine, num_cu=256, critic=False, candidates=None, node_output=False, per_instance=False, obs_f64=False,
                     single_ok=True, reduce=False, product_mode=0, rows=None):
    """Which path a GIN forward takes, who pools and every launch it makes — the library's own rule (csrc/mtfjsp_gin_select.h), no GPU needed.
    critic: the global critic asks (no candidates) instead of the job actor; candidates: per instance (default n_job, 0 for the critic);
    single_ok, reduce, product_mode: the handle's answers (its census passed; a statistics reduction is installed; its product mode); rows: rows per
    instance where they are not n_job * n_machine.  The streaming switches (MTFJSP_FUSE_GIN0, MTFJSP_FUSE_POOL, MTFJSP_FUSE_PAIR, MTFJSP_NO_STREAM_ORDER,
    MTFJSP_STREAM_NT, MTFJSP_POOL_S, MTFJSP_FUSE_POOL_MAXT), MTFJSP_NO_RESIDENT_GIN and MTFJSP_GIN_RES_GENERIC are read from the environment per call
    (defaults: csrc/mtfjsp_enc_switches.h, the table "Encoder switches" of DESIGN.md)."""
    flags = (GIN_CRITIC * bool(critic) | GIN_NODE_OUTPUT * bool(node_output) | GIN_PER_INSTANCE * bool(per_instance) | GIN_OBS_F64 * bool(obs_f64) |
             GIN_NO_SINGLE * (not single_ok) | GIN_REDUCE * bool(reduce))
    J = (0 if critic else n_job) if candidates is None else candidates
    T = n_job * n_machine if rows is None else rows
    return _gin_launches(lambda *out: lib().mtfjsp_gin_launches_for(batch, T, n_job, J, num_cu, product_mode, flags, *out))


def encoder_gin_launches(handle):
    """the same report for the handle's last GIN forward (None: none yet)"""
    return _gin_launches(lambda *out: lib().mtfjsp_encoder_gin_launches(handle, *out))


def fused3_kernel_for(batch, n_job, n_machine, num_cu=256, obs_f64=False, env_tail=False):
    """(kernel name or None, workgroups): which instantiation of the three-in-one heads launch serves a rollout step of this shape — the library's
    own rule (csrc/mtfjsp_fused3_select.h), no GPU needed.  MTFJSP_FUSED3_GENERIC=1 in the environment forces the run-time kernel."""
    grid = C.c_int32(0)
    name = lib().mtfjsp_fused3_kernel_name_for(batch, n_job, n_machine, num_cu, int(bool(obs_f64)), int(bool(env_tail)), C.byref(grid))
    return (name.decode() if name else None), grid.value


# flag bits of mtfjsp_heads_kernel_name_for (include/mtfjsp.h)
HEADS_GAT, HEADS_MHEADS, HEADS_ENV_TAIL, HEADS_VALUES_ONLY, HEADS_F32, HEADS_NO_GAT, HEADS_NO_MHEADS, HEADS_OBS_F64 = 1, 2, 4, 8, 16, 32, 64, 128


def heads_kernel_for(batch, n_job, n_machine, which=0, num_cu=256, gat=False, mheads=False, env_tail=False, values_only=False, f32=False,
                     gat_ok=True, mheads_ok=True, obs_f64=False):
    """(kernel name, instances per workgroup, workgroups): which heads kernel serves the job (which = 0) / machine (which = 1) actor's forward — the
    library's own rule (csrc/mtfjsp_heads_select.h), no GPU needed.  gat / mheads / env_tail / values_only: what the caller asks to ride in the launch;
    f32, gat_ok, mheads_ok: the handle's answers (product mode bit 4; its half of the two fusion conditions).  MTFJSP_NO_HEADS_HG8, MTFJSP_NO_HEADS10,
    MTFJSP_FUSED3_NODES_HBM and MTFJSP_FUSED3_GENERIC are read from the environment per call (csrc/mtfjsp_enc_switches.h)."""
    flags = (HEADS_GAT * bool(gat) | HEADS_MHEADS * bool(mheads) | HEADS_ENV_TAIL * bool(env_tail) | HEADS_VALUES_ONLY * bool(values_only) |
             HEADS_F32 * bool(f32) | HEADS_NO_GAT * (not gat_ok) | HEADS_NO_MHEADS * (not mheads_ok) | HEADS_OBS_F64 * bool(obs_f64))
    group, grid = C.c_int32(0), C.c_int32(0)
    name = lib().mtfjsp_heads_kernel_name_for(batch, n_machine if which else n_job, n_machine, n_job * n_machine, num_cu, flags, C.byref(group), C.byref(grid))
    return (name.decode() if name else None), group.value, grid.value
