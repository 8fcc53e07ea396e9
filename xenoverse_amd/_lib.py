"""ctypes binding of libxeno_hip.so (C-ABI: include/xeno.h).

There is NO fallback: if the HIP library is missing or does not load, importing the engine raises.  The
product never computes an environment step on the CPU.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# XV_LIB_PATH: A/B measurement of kernel variants built by scripts/devtools/build_variant.py (same ABI, same checks)
LIB_PATH = os.environ.get("XV_LIB_PATH") or os.path.join(_HERE, "libxeno_hip.so")

c_void_p, c_int, c_u64, c_i64, c_u32 = C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_uint32

# name -> argtypes (restype is int unless listed in _RESTYPE).  Keep in sync with include/xeno.h;
# tests/test_abi.py parses the header and checks that every declared symbol is exported and bound.
SIGNATURES = {
    "xv_abi_version": [],
    "xv_pack_rollout": [c_void_p, C.c_size_t] + [c_void_p] * 6,
    "xv_unpack_rollout": [c_void_p, C.c_size_t] + [c_void_p] * 6,
    "xv_pack_rollout_f32": [c_void_p, C.c_size_t, c_int] + [c_void_p] * 6,
    "xv_unpack_rollout_f32": [c_void_p, C.c_size_t, c_int] + [c_void_p] * 6,
    "xv_last_error": [],
    "xv_rccl_unique_id": [c_void_p],
    "xv_rccl_comm_create": [c_void_p, c_int, c_int, c_void_p, C.POINTER(c_void_p)],
    "xv_rccl_comm_destroy": [c_void_p],
    "xv_rccl_comm_count": [c_void_p, C.POINTER(c_int)],
    "xv_rollout_allgather": [c_void_p, c_void_p, c_void_p, c_void_p, C.c_size_t],
    "xv_engine_create": [c_int, c_u64, c_u64, c_void_p, C.POINTER(c_void_p)],
    "xv_engine_destroy": [c_void_p],
    "xv_engine_sync": [c_void_p],
    "xv_engine_stream": [c_void_p],
    "xv_engine_error_flags": [c_void_p, c_int, C.POINTER(c_u32)],
    "xv_engine_get_tick": [c_void_p, C.POINTER(c_u64)],
    "xv_engine_set_tick": [c_void_p, c_u64],
    "xv_engine_set_device_tick": [c_void_p, c_int],
    "xv_engine_device_tick": [c_void_p],
    "xv_engine_tick_batch": [c_void_p, c_int],
    "xv_engine_set_stream": [c_void_p, c_void_p],
    "xv_engine_event_record": [c_void_p, c_int],
    "xv_engine_event_done": [c_void_p, c_int, C.POINTER(c_int)],
    "xv_engine_event_elapsed_ms": [c_void_p, C.POINTER(C.c_float)],
    "xv_philox4x32_10": [c_void_p, c_void_p, c_void_p, c_void_p, c_int],
    "xv_anymdp_create": [c_void_p, c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 7 + [C.POINTER(c_void_p)],
    "xv_anymdp_destroy": [c_void_p],
    "xv_anymdp_reset": [c_void_p, c_void_p, c_void_p],
    "xv_anymdp_reset_injected": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anymdp_step": [c_void_p] + [c_void_p] * 7 + [c_int],
    "xv_anymdp_step_info": [c_void_p] + [c_void_p] * 9 + [c_int],
    "xv_anymdp_step_injected": [c_void_p] + [c_void_p] * 10 + [c_int],
    "xv_anymdp_step_many": [c_void_p, c_int, c_int] + [c_void_p] * 7 + [c_int],
    "xv_anymdp_set_step_many_graph": [c_void_p, c_int],
    "xv_anymdp_set_step_many_overlap": [c_void_p, c_int],
    "xv_anymdp_step_many_overlap_state": [c_void_p],
    "xv_anymdp_build_rows": [c_void_p, c_int, c_int, c_int] + [c_void_p] * 6 + [c_u64],
    "xv_anymdp_view": [c_void_p, c_void_p, c_int, c_int, C.POINTER(c_void_p)],
    "xv_anymdp_step_many_chains": [c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 7 + [c_int],
    "xv_anymdp_solve": [c_void_p, C.c_double, C.c_double, c_int, c_void_p, c_void_p, c_void_p],
    "xv_anymdp_step_many_graph_state": [c_void_p],
    "xv_anymdp_sample_tasks": [c_void_p, c_u64, c_i64, c_int, c_int, c_int, c_int] + [c_void_p] * 11,
    "xv_anymdp_sample_garnet": [c_void_p, c_u64, c_i64, c_int, c_int, c_int, c_int, c_int, C.c_double, c_int] + [c_void_p] * 10,
    "xv_anymdp_sample_bandits": [c_void_p, c_u64, c_i64, c_int, c_int, c_int, c_int] + [c_void_p] * 9,
    "xv_anymdp_value_iteration_set_summation": [c_int],
    "xv_anymdp_sample_observation_model": [c_void_p, c_u64, c_i64, c_int, c_int, c_int, c_int, C.c_double, C.c_double, c_void_p],
    "xv_anymdp_value_iteration_gs": [c_void_p, c_void_p, c_int, c_int, C.c_double, c_int, c_void_p, c_void_p],
    "xv_anymdp_rollout": [c_void_p, c_int] + [c_void_p] * 7,
    "xv_anymdp_set_search": [c_void_p, c_int],
    "xv_anymdp_build_buckets": [c_void_p, c_int],
    "xv_anymdp_probe_buckets": [c_void_p, c_int, c_void_p],
    "xv_anymdp_bucket_census_get": [c_void_p, c_void_p],
    "xv_anymdp_effective_search": [c_void_p],
    "xv_anymdp_token_kernel": [c_void_p],
    "xv_anymdp_set_observation_model": [c_void_p, c_int, c_int, c_int, c_void_p],
    "xv_anymdp_reset_tokens": [c_void_p, c_void_p, c_void_p],
    "xv_anymdp_reset_tokens_injected": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anymdp_step_tokens": [c_void_p] + [c_void_p] * 7 + [c_int],
    "xv_anymdp_step_tokens_info": [c_void_p] + [c_void_p] * 9 + [c_int],
    "xv_anymdp_step_tokens_injected": [c_void_p] + [c_void_p] * 12 + [c_int],
    "xv_anymdp_step_tokens_many": [c_void_p, c_int, c_int] + [c_void_p] * 7 + [c_int],
    "xv_anymdp_rollout_teacher": [c_void_p, c_int, c_void_p, C.c_float] + [c_void_p] * 7,
    "xv_anymdp_rollout_tokens": [c_void_p, c_int] + [c_void_p] * 7,
    "xv_anymdp_rollout_tokens_teacher": [c_void_p, c_int, c_void_p, C.c_float] + [c_void_p] * 7,
    "xv_anymdp_qlearn_create": [c_void_p, C.c_double, C.c_double, c_int, C.POINTER(c_void_p)],
    "xv_anymdp_qlearn_destroy": [c_void_p],
    "xv_anymdp_qlearn_reset": [c_void_p, c_void_p],
    "xv_anymdp_qlearn_get_state": [c_void_p] * 4,
    "xv_anymdp_qlearn_set_state": [c_void_p] * 4,
    "xv_anymdp_rollout_qlearn": [c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 11,
    "xv_anymdp_mbrl_create": [c_void_p, C.c_double, C.c_double, C.POINTER(c_void_p)],
    "xv_anymdp_mbrl_destroy": [c_void_p],
    "xv_anymdp_mbrl_reset": [c_void_p, c_void_p],
    "xv_anymdp_mbrl_get_state": [c_void_p] * 6,
    "xv_anymdp_mbrl_set_state": [c_void_p] * 6,
    "xv_anymdp_rollout_mbrl": [c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 11,
    "xv_anymdp_get_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anymdp_set_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anymdp_transition_gt": [c_void_p, c_void_p, c_void_p],
    "xv_anymdp_synth_tasks": [c_void_p, c_u64, c_i64, c_int, c_int, c_int, c_int] + [c_void_p] * 6,
    "xv_mixed_step": [c_void_p, c_void_p, c_void_p, c_void_p, c_int],
    "xv_mixed_supported": [c_void_p, c_void_p, c_void_p],
    "xv_mixed_step_many": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int],
    "xv_mixed_step_many_overlap_state": [c_void_p],
    "xv_engine_probe_side_streams": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_linds_create": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, C.POINTER(c_void_p)],
    "xv_linds_destroy": [c_void_p],
    "xv_linds_step_many": [c_void_p, c_int, c_int] + [c_void_p] * 8 + [c_int],
    "xv_linds_set_path": [c_void_p, c_int],
    "xv_linds_set_command_table": [c_void_p, c_int],
    "xv_linds_reset": [c_void_p] + [c_void_p] * 4,
    "xv_linds_reset_injected": [c_void_p] + [c_void_p] * 5,
    "xv_linds_step": [c_void_p] + [c_void_p] * 8 + [c_int],
    "xv_linds_step_info": [c_void_p] + [c_void_p] * 10 + [c_int],
    "xv_linds_step_injected": [c_void_p] + [c_void_p] * 10 + [c_int],
    "xv_linds_rollout": [c_void_p, c_int] + [c_void_p] * 8,
    "xv_linds_get_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_linds_set_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_linds_mpc_create": [c_void_p, c_int, C.c_double, c_void_p, c_int, C.POINTER(c_void_p)],
    "xv_linds_mpc_destroy": [c_void_p],
    "xv_linds_mpc_action": [c_void_p] * 5,
    "xv_linds_mpc_solve": [c_void_p] + [c_void_p] * 5,
    "xv_linds_rollout_mpc": [c_void_p, c_int] + [c_void_p] * 10,
    "xv_linds_sample_tasks": [c_void_p, c_u64, c_i64] + [c_int] * 9 + [C.c_double, c_i64] + [c_void_p] * 4,
    "xv_linds_build_zoh": [c_void_p, c_int, c_void_p, c_int, c_int] + [c_void_p] * 3 + [C.c_double] + [c_void_p] * 6,
    "xv_maze_create": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, C.c_double, C.c_double,
                       c_void_p, c_void_p, C.POINTER(c_void_p)],
    "xv_maze_destroy": [c_void_p],
    "xv_maze_reset": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_maze_step": [c_void_p, c_void_p, c_int] + [c_void_p] * 6 + [c_int],
    "xv_maze_get_state": [c_void_p] + [c_void_p] * 8,
    "xv_maze_set_state": [c_void_p] + [c_void_p] * 6,
    "xv_maze_render": [c_void_p, c_void_p, c_void_p],
    "xv_maze_set_precision": [c_void_p, c_int],
    "xv_maze_set_raycast_mapping": [c_void_p, c_int],
    "xv_maze_set_typing": [c_void_p, c_int],
    "xv_maze_set_move_kernel": [c_void_p, c_int],
    "xv_maze_sample_tasks": [c_void_p, c_u64, c_i64, c_int, c_int] + [c_void_p] * 4,
    "xv_maze_sampler_check": [c_i64, c_int, c_int] + [c_void_p] * 3,
    "xv_maze_resample_tasks": [c_void_p, c_u64, c_i64, c_i64] + [c_int] * 4 + [c_void_p],
    "xv_maze_agent_create": [c_void_p, c_int, C.c_double, c_int, c_int, c_int, c_void_p],
    "xv_maze_agent_destroy": [c_void_p],
    "xv_maze_agent_act": [c_void_p, c_void_p, c_void_p],
    "xv_maze_agent_get": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_maze_set_episode_resample": [c_void_p, c_int, c_u64, c_i64, c_i64, c_void_p, c_void_p],
    "xv_maze_rollout_check": [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, C.c_double],
    "xv_maze_rollout": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "xv_maze_rollout_agent": [c_void_p, c_void_p, c_int, C.c_double, c_int, c_void_p],
    "xv_metalang_create": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_void_p)],
    "xv_metalang_destroy": [c_void_p],
    "xv_metalang_set_task": [c_void_p, c_int] + [c_void_p] * 8,
    "xv_metalang_generate": [c_void_p, c_int, c_void_p, c_void_p, c_void_p],
    "xv_metalang_log_prob": [c_void_p, c_int, c_void_p, c_void_p],
    "xv_metalang_describe": [c_void_p, c_int, c_void_p],
    "xv_metalang1_create": [c_void_p, c_int, C.POINTER(c_void_p)],
    "xv_metalang1_destroy": [c_void_p],
    "xv_metalang1_set_task": [c_void_p, c_int, c_int, c_int] + [c_void_p] * 6,
    "xv_metalang1_generate": [c_void_p, c_int, C.c_double, c_void_p, c_int] + [c_void_p] * 7,
    "xv_metalang_sample_tasks": [c_void_p, c_u64, c_i64] + [c_int] * 4 + [c_void_p, c_int, c_int, C.c_double] + [c_void_p] * 7,
    "xv_metalang1_sample_lengths": [c_void_p, c_u64, c_i64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
    "xv_metalang1_sample_offsets": [c_void_p, c_int, c_int] + [c_void_p] * 4,
    "xv_metalang1_sample_tokens": [c_void_p, c_u64, c_i64, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p],
    "xv_metalm_create": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, C.POINTER(c_void_p)],
    "xv_metalm_destroy": [c_void_p],
    "xv_metalm_set_task": [c_void_p, c_int] + [c_void_p] * 6,
    "xv_metalm_reset": [c_void_p] + [c_void_p] * 3,
    "xv_metalm_policy": [c_void_p] + [c_void_p] * 4,
    "xv_metalm_step": [c_void_p] + [c_void_p] * 16,
    "xv_metalm_get_state": [c_void_p] * 5,
    "xv_metalm_set_state": [c_void_p] * 5,
    "xv_metalm_stream": [c_void_p, c_int, c_int, c_int, c_void_p, c_int] + [c_void_p] * 12,
    "xv_metalm_sample_tasks": [c_void_p, c_u64, c_i64] + [c_int] * 6 + [c_void_p, c_int] + [c_void_p] * 14,
    "xv_anyhvac_create": [c_void_p] + [c_int] * 9 + [C.c_double] * 4 + [c_int, C.POINTER(c_void_p)],
    "xv_anyhvac_destroy": [c_void_p],
    "xv_anyhvac_set_task": [c_void_p, c_int, c_void_p, c_void_p],
    "xv_anyhvac_reset": [c_void_p, c_void_p, c_void_p],                 # (handle, mask, xv_anyhvac_io*)
    "xv_anyhvac_reset_injected": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anyhvac_step": [c_void_p, c_void_p, c_int],
    "xv_anyhvac_step_injected": [c_void_p, c_void_p, c_void_p, c_int],
    "xv_anyhvac_rollout": [c_void_p, c_int, c_void_p, c_int],
    "xv_anyhvac_get_state": [c_void_p, c_void_p],                       # (handle, xv_anyhvac_state*)
    "xv_anyhvac_set_state": [c_void_p, c_void_p],
    "xv_anyhvac_set_pid": [c_void_p, c_void_p, c_void_p, c_int],            # (handle, weights, gains, kind_flags)
    "xv_anyhvac_pid_action": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anyhvac_rollout_pid": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int],
    "xv_anyhvac_pid_get_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anyhvac_pid_set_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anyhvac_pid_reset": [c_void_p, c_void_p],
    "xv_anyhvac_set_action_mode": [c_void_p, c_int, c_int, c_void_p],       # (handle, mode, flags, host cost table)
    "xv_anyhvac_step_mapped": [c_void_p, c_void_p, c_void_p, c_int],        # (handle, xv_anyhvac_io*, xv_anyhvac_act_io*, mode)
    "xv_anyhvac_step_mapped_injected": [c_void_p, c_void_p, c_void_p, c_void_p, c_int],
    "xv_anyhvac_rollout_mapped": [c_void_p, c_int, c_void_p, c_void_p, c_int],
    "xv_anyhvac_act_get_state": [c_void_p, c_void_p],
    "xv_anyhvac_act_set_state": [c_void_p, c_void_p],
    "xv_anyhvac_set_start_mode": [c_void_p, c_void_p, c_i64, c_void_p, c_i64],  # (handle, host flags, max_steps, host cdf, n)
    "xv_anyhvac_set_start_draws": [c_void_p, c_void_p],
    "xv_anyhvac_start_get_state": [c_void_p, c_void_p, c_void_p, c_void_p],     # (handle, last_fail, ring, count)
    "xv_anyhvac_start_set_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    "xv_anyhvac_sample_tasks": [c_void_p, c_u64, c_i64] + [c_int] * 8 + [c_void_p] * 5,
    "xv_chem_create": [c_void_p, c_int, C.POINTER(c_void_p)],
    "xv_chem_destroy": [c_void_p],
    "xv_chem_set_worlds": [c_void_p, c_int, c_int, c_int] + [c_void_p] * 9,
    "xv_chem_simulate": [c_void_p, c_int] + [c_void_p] * 10 + [C.c_double, c_void_p],
    "xv_chem_optimal": [c_void_p] + [c_int] * 4 + [c_void_p] * 13 + [C.c_double, c_void_p, c_void_p],
    "xv_anyhvac_sampler_check": [c_i64] + [c_int] * 8 + [c_void_p] * 4,
}
for _p in ("xv_cartpole", "xv_acrobot"):      # the control families share one set of entry points (csrc/xv_control.h)
    SIGNATURES.update({
        # acrobot's extra int: scale_is_vector
        _p + "_create": [c_void_p] + [c_int] * 4 + [c_void_p] * 2 + [c_int] * (_p == "xv_acrobot") + [c_void_p, C.POINTER(c_void_p)],
        _p + "_destroy": [c_void_p],
        _p + "_reset": [c_void_p, c_void_p, c_void_p],
        _p + "_reset_injected": [c_void_p, c_void_p, c_void_p, c_void_p],
        _p + "_step": [c_void_p] + [c_void_p] * 6 + [c_int],
        _p + "_step_info": [c_void_p] + [c_void_p] * 7 + [c_int],
        _p + "_rollout": [c_void_p, c_int] + [c_void_p] * 6 + [c_int],
        _p + "_step_injected": [c_void_p] + [c_void_p] * 7 + [c_int],
        _p + "_get_state": [c_void_p, c_void_p, c_void_p, c_void_p],
        _p + "_set_state": [c_void_p, c_void_p, c_void_p, c_void_p],
    })
_RESTYPE ={"xv_last_error": C.c_char_p, "xv_engine_stream": c_void_p}

_lib = None


class BucketCensus(C.Structure):
    """xv_anymdp_bucket_census (include/xeno.h)"""
    _fields_ = [("n_bucket", C.c_int32), ("format", C.c_int32), ("cuts_per_line", C.c_int32), ("built", C.c_int32),
                ("auto_uses_bucket", C.c_int32), ("reserved", C.c_int32), ("lines", C.c_uint64), ("lines_dirty", C.c_uint64),
                ("live_rows", C.c_uint64), ("p_fallback", C.c_double), ("fallbacks_per_launch", C.c_double),
                ("bytes", C.c_double), ("auto_limit", C.c_double), ("obs_lines", C.c_uint64), ("obs_lines_dirty", C.c_uint64),
                ("obs_p_fallback", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class AnyHVACIO(C.Structure):
    """xv_anyhvac_io (include/xeno.h): device pointers of what a step reads and writes"""
    FIELDS = ("action", "sensor_readings", "heat_readings", "action_temp", "timestep", "reward", "terminated", "truncated",
              "final_sensor_readings", "final_heat_readings", "final_action_temp", "final_timestep", "cool_power",
              "heat_power", "misc")
    _fields_ = [(k, C.c_void_p) for k in FIELDS]


class AnyHVACState(C.Structure):
    """xv_anyhvac_state (include/xeno.h)"""
    FIELDS = ("grid", "t", "last_call", "episode_step", "warning_count", "rest_idx", "rest_start", "value", "filter",
              "ring_t", "ring_v", "head", "tail")
    _fields_ = [(k, C.c_void_p) for k in FIELDS]


class AnyHVACActIO(C.Structure):
    """xv_anyhvac_act_io (include/xeno.h)"""
    FIELDS = ("action_index", "applied_value", "delta", "action_cost", "stat_counts")
    _fields_ = [(k, C.c_void_p) for k in FIELDS]


class ChemOut(C.Structure):
    """xv_chem_out (include/xeno.h): device pointers of what a ChemVerse launch writes, each nullable"""
    FIELDS = ("final_pool", "consumed", "produced", "byproduct", "gas_lost", "fired", "num_steps", "steps_run", "converged",
              "failure", "failure_step", "final_T", "final_P", "hist_step", "hist_T", "hist_P", "hist_count", "log_step",
              "log_active", "log_T", "log_P", "log_consumed", "log_produced", "log_count")
    _fields_ = [(k, C.c_void_p) for k in FIELDS]


class ChemOptOut(C.Structure):
    """xv_chem_opt_out (include/xeno.h): device pointers of what xv_chem_optimal writes, each nullable"""
    FIELDS = ("best_scale", "found", "bits", "yield", "charged", "consumed", "produced", "byproduct", "final_pool", "failure")
    _fields_ = [(k, C.c_void_p) for k in FIELDS]


class XenoError(RuntimeError):
    code = 0      # the XV_ERR_* value check() saw (include/xeno.h)


XV_ERR_INVALID, XV_ERR_HIP, XV_ERR_UNSUPPORTED, XV_ERR_NOMEM = -1, -2, -3, -4


ABI_VERSION = 12     # include/xeno.h XV_ABI_VERSION


def load():
    """Load libxeno_hip.so; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XenoError(
            "libxeno_hip.so is not built (%s). Run `python -m xenoverse_amd.build` (needs hipcc). "
            "xenoverse_amd has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing: loud by design
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, c_int)
    if lib.xv_abi_version() != ABI_VERSION:
        raise XenoError("libxeno_hip.so has ABI version %d, this package binds version %d: rebuild with "
                        "`python -m xenoverse_amd.build --force`" % (lib.xv_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


_fast = [None, False]      # (module or None, tried)


def fast():
    """the CPython trampoline `_xvfast` (xenoverse_amd/_xvfast.so, built by xenoverse_amd.build.build_fast) or None: a shortcut
    for the BINDING of a few hot calls — ctypes serves the same C-ABI without it (XV_NO_FAST=1 forces that)"""
    if not _fast[1]:
        _fast[1] = True
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_xvfast.so")
        if os.path.exists(path) and not os.environ.get("XV_NO_FAST"):
            try:
                import importlib.util
                spec = importlib.util.spec_from_file_location("_xvfast", path)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                _fast[0] = mod
            except Exception:
                _fast[0] = None
    return _fast[0]


def fn_address(name):
    """address of a C-ABI entry point (for _xvfast.icall)"""
    return C.cast(getattr(load(), name), C.c_void_p).value


_step_fns = {}      # name -> (_xvfast.icall or None, address, ctypes function)


def step_call(name, h, action, outputs, mode):
    """THE hot call of every family: `name`(h, action, *outputs' pointers in the C call's order, mode) — through the
    trampoline when it is built, through ctypes otherwise.  outputs: a vector.OutputSet."""
    e = _step_fns.get(name)
    if e is None:
        f = fast()
        e = _step_fns[name] = (f.icall if f is not None else None, fn_address(name), getattr(load(), name))
    icall, address, fn = e
    if icall is not None:
        rc = icall(address, h.value, action.data_ptr(), *outputs.ints, mode)
    else:
        rc = fn(h, C.c_void_p(action.data_ptr()), *outputs.args, mode)
    if rc:
        check(rc)


def check(rc):
    if rc != 0:
        msg = load().xv_last_error()
        err = XenoError("libxeno_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        err.code = int(rc)
        raise err


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    if t is None:
        return None
    assert t.is_contiguous(), "tensors handed to the C-ABI must be contiguous"
    return t.data_ptr()
