// maze_rollout.hip — MazeWorld fused rollouts (T vector steps issued by one C call, every result stacked over T) and
// resampled episodes (the reference's Resampler applied to an env's task at every reset of that env, on the device).
//
// Reference: the data-collection loops around MazeWorldEnvBase.step (xenoverse/mazeworld/envs/maze_env.py:50-66) and the
// agents' step (xenoverse/mazeworld/agents/agent_base.py): `action = agent.step(obs, r); obs, r, te, tr, info =
// env.step(action)`, each episode started by `env.set_task(Resampler(task)); env.reset()` (resample_task,
// envs/task_sampler.py:179-225).  The launches are those of xv_maze_agent_act and xv_maze_step, in the loop's order
// (maze_common.h maze_agent_launch / maze_launch_move / maze_launch_render), so a rollout is the loop bit for bit; new is
//   * the move kernels write reward and flags into row t of the caller's [T][n_env] tensors,
//   * maze_poststep_kernel, one wave per env after the move: for an env the move launch reset (fin_flag) it runs the
//     Resampler on the env's task (ms_resample_task, shared with xv_maze_resample_tasks) and places the agent at the new
//     start; then it writes the rest of row t — the trajectory record and the `command` RGB that otherwise only the ray
//     caster writes — so a rollout without frames never launches the ray caster,
//   * frames are painted straight into their row of the [T / s] stack.
// `steps` is the count BEFORE the step (the info["steps"] quirk of maze_env.py:57): row 0 is a copy of the state, row t + 1
// is written by the per-step kernel of step t.  No loop of the kernel depends on data for its end: the Resampler's are
// bounded by the landmark count (<= 15), the cell count and n_cmd (maze_sampler.hip).
#include "maze_common.h"

#ifdef XV_KERNELS_ONLY
#include "maze_sampler.hip"
#else
#define XV_KERNELS_ONLY      // the sampler's kernels and device functions, not its C-ABI
#include "maze_sampler.hip"
#undef XV_KERNELS_ONLY
#endif

struct MzEpisode {        // resampled episodes; re.flags == 0: off (and no LDS is asked for)
  MsReArgs re;            // slots = the env's own tables (one task per env); re.episode unused
  int64_t episode_base;
  int32_t* episodes;      // [n_env] resets so far
};

// One wave per env.  is_reset: the resampling reset itself (xv_maze_reset's mask semantics, no record).
__global__ __launch_bounds__(64) void maze_poststep_kernel(MazeArgs P, MzRow R, MzEpisode E, int is_reset, const uint8_t* mask) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mzr_lds[];
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= P.n_env) return;
  const size_t N = (size_t)P.n_env, se = (size_t)e;
  const int t = P.env_task[e];
  int episode = 0;
  if (E.re.flags != 0) {
    const bool restart = is_reset ? (mask == nullptr || mask[e] != 0) : P.fin_flag[e] != 0;      // the same for the whole wave
    episode = E.episodes[e];
    if (restart) {
      const int64_t ep = E.episode_base + (int64_t)episode;
      if (ep < ((int64_t)1 << 24)) ms_resample_task(*reinterpret_cast<MsLds*>(mzr_lds), E.re, t, (uint32_t)ep);
      else if (lane == 0) atomicOr(P.err, XV_DEVERR_EPISODE_RANGE);      // refused, as xv_maze_resample_tasks refuses it: the task stays
      __syncthreads();      // the new start and commands are visible to the wave
      if (lane == 0) {
        mz_reset_env(P, e, t);
        E.episodes[e] = episode + 1;
      }
      ++episode;
      __syncthreads();
    }
  }
  if (is_reset || R.pos == nullptr) return;
  switch (lane) {      // the fields of the row are dealt to the lanes
    case 0: R.pos[2 * se] = P.pos[e]; break;
    case 1: R.pos[2 * se + 1] = P.pos[N + e]; break;
    case 2: R.ori[e] = P.ori[e]; break;
    case 3: R.grid[2 * se] = P.grid[e]; break;
    case 4: R.grid[2 * se + 1] = P.grid[N + e]; break;
    case 5: R.cmd_idx[e] = P.cmd_idx[e]; break;
    case 6: R.cmd_age[e] = P.cmd_age[e]; break;
    case 7: R.collision[e] = P.collision[e]; break;
    case 8: R.episode[e] = episode; break;
    case 9: if (R.steps_next != nullptr) R.steps_next[e] = P.steps[e]; break;
    case 10: case 11: case 12:
      if (R.final_pose != nullptr) R.final_pose[3 * se + (lane - 10)] = P.fin_flag[e] ? P.fin_pose[(size_t)(lane - 10) * N + e] : 0.0;
      break;
    case 16: case 17: case 18: case 19: {   // the commanded landmark, as the ray caster reads it (maze.hip maze_raycast_kernel)
      const int idx = P.cmd_idx[e];
      const int cmd = P.T.commands[(size_t)t * P.n_cmd + (idx < P.n_cmd ? idx : P.n_cmd - 1)];
      if (lane == 19) R.target[e] = cmd;
      else R.command[3 * se + (lane - 16)] = MZ_LANDMARK_RGB[cmd < 0 ? 0 : (cmd >= XV_MAZE_LMAX ? XV_MAZE_LMAX - 1 : cmd)][lane - 16];
      break;
    }
    default: break;
  }
}

#ifndef XV_KERNELS_ONLY

int maze_launch_poststep(xv_maze* h, const MzRow& R, bool is_reset, const uint8_t* reset_mask) {
  const MazeArgs& a = h->a;
  MzEpisode E{};
  E.re.flags = h->re_flags;
  if (h->re_flags != 0) {
    E.re.seed = h->re_seed; E.re.index_base = h->re_index_base; E.re.n_task = a.n_task; E.re.NG = a.NG; E.re.n_cmd = a.n_cmd;
    // the tables the env reads ARE the slots: xv_maze_set_episode_resample made them the env's private, writable copies
    E.re.o.walls = const_cast<int8_t*>(a.T.walls); E.re.o.landmarks = const_cast<int8_t*>(a.T.landmarks);
    E.re.o.ints = const_cast<int32_t*>(a.T.ints); E.re.o.commands = const_cast<int32_t*>(a.T.commands);
    E.re.o.lm_coord = const_cast<int32_t*>(a.T.lm_coord);
    E.episode_base = h->re_episode_base; E.episodes = h->re_episodes;
  }
  hipLaunchKernelGGL(maze_poststep_kernel, dim3(a.n_env), dim3(64), h->re_flags != 0 ? sizeof(MsLds) : 0, h->eng->stream, a, R, E,
                     is_reset ? 1 : 0, reset_mask);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_maze_set_episode_resample(xv_maze* h, int flags, uint64_t seed, int64_t index_base, int64_t episode_base,
                                            const xv_maze_task_slots* own, int32_t* episodes) {
  XV_CHECK_ARG(h != nullptr);
  XV_CHECK_ARG((flags & ~(XV_MAZE_RESAMPLE_CMD | XV_MAZE_RESAMPLE_START | XV_MAZE_RESAMPLE_LANDMARKS | XV_MAZE_RESAMPLE_COLOR)) == 0);
  if (flags == 0) {
    h->re_flags = 0;
    return XV_OK;
  }
  MazeArgs& a = h->a;
  XV_CHECK_ARG(own != nullptr && episodes != nullptr);
  XV_CHECK_ARG(own->landmarks && own->ints && own->commands && own->lm_coord);
  XV_CHECK_ARG(a.n_task == a.n_env);      // one task per env (the caller checks that env_task is a permutation)
  XV_CHECK_ARG(index_base >= 0 && episode_base >= 0 && episode_base < ((int64_t)1 << 24));
  XV_CHECK_ARG(a.NG >= 3 && a.NG <= MS_N_MAX + 1 && a.n_cmd >= 1 && a.n_cmd <= MS_CMD_MAX);
  XV_HIP(hipSetDevice(h->eng->device));
  XV_HIP(hipMemsetAsync(episodes, 0, sizeof(int32_t) * (size_t)a.n_env, h->eng->stream));
  a.T.landmarks = own->landmarks; a.T.ints = own->ints; a.T.commands = own->commands; a.T.lm_coord = own->lm_coord;
  h->re_flags = flags; h->re_seed = seed; h->re_index_base = index_base; h->re_episode_base = episode_base;
  h->re_episodes = episodes;
  return XV_OK;
}

extern "C" int xv_maze_rollout_check(int n_env, int action_mode, int autoreset_mode, int T, int frame_stride,
                                     const void* actions, const xv_maze_rollout_out* out, int with_agent, double epsilon) {
  XV_CHECK_ARG(out != nullptr);
  XV_CHECK_ARG(n_env > 0 && T >= 1 && frame_stride >= 0);
  XV_CHECK_ARG(action_mode >= 0 && action_mode <= 2 && autoreset_mode >= 0 && autoreset_mode <= 2);
  XV_CHECK_ARG(out->reward && out->terminated && out->truncated && out->steps && out->command);
  XV_CHECK_ARG(out->pos && out->ori && out->grid && out->cmd_idx && out->cmd_age && out->collision && out->target &&
               out->episode);
  const bool painted = frame_stride > 0 && T / frame_stride > 0;
  XV_CHECK_ARG((out->frames != nullptr) == painted);
  XV_CHECK_ARG(out->final_frames == nullptr || (painted && autoreset_mode == XV_AUTORESET_SAME_STEP));
  XV_CHECK_ARG(out->final_pose == nullptr || autoreset_mode == XV_AUTORESET_SAME_STEP);
  if (with_agent) {
    XV_CHECK_ARG(actions == nullptr && out->action && out->action_label && out->explored);
    XV_CHECK_ARG(action_mode == XV_MAZE_ACTION_DISCRETE16 || action_mode == XV_MAZE_ACTION_DISCRETE32);
    XV_CHECK_ARG(autoreset_mode == XV_AUTORESET_SAME_STEP);
    XV_CHECK_ARG(epsilon >= 0.0 && epsilon <= 1.0);      // (a NaN fails both)
  } else {
    XV_CHECK_ARG(actions != nullptr);
  }
  return XV_OK;
}

// the T steps of either call: g null = the actions are given
static int maze_rollout_steps(xv_maze* h, xv_maze_agent* g, xv_maze_agent* label, const void* actions, int action_mode, int T,
                              int frame_stride, int mode, double epsilon, const xv_maze_rollout_out& o) {
  const MazeArgs& a = h->a;
  const size_t n = (size_t)a.n_env, fsz = n * (size_t)a.W * a.H * 3;
  const size_t act_bytes = action_mode == XV_MAZE_ACTION_CONTINUOUS ? 16 : 4;
  hipStream_t s = h->eng->stream;
  XV_HIP(hipSetDevice(h->eng->device));
  XV_HIP(hipMemcpyAsync(o.steps, a.steps, 4 * n, hipMemcpyDeviceToDevice, s));
  for (int t = 0; t < T; ++t) {
    const size_t r = (size_t)t * n;
    const void* act = g != nullptr ? nullptr : static_cast<const uint8_t*>(actions) + r * act_bytes;
    if (g != nullptr) {
      int rc = maze_agent_launch(g, nullptr, o.action + r, MazeExplore{epsilon, label ? nullptr : o.action_label + r, o.explored + r});
      if (rc == XV_OK && label != nullptr)
        rc = maze_agent_launch(label, nullptr, o.action_label + r, MazeExplore{0.0, nullptr, nullptr});
      if (rc != XV_OK) return rc;
      act = o.action + r;
    }
    int rc = maze_launch_move(h, act, action_mode, o.reward + r, o.terminated + r, o.truncated + r, mode);
    if (rc != XV_OK) return rc;
    const bool paint = frame_stride > 0 && (t + 1) % frame_stride == 0;
    const size_t k = paint ? (size_t)((t + 1) / frame_stride - 1) : 0;
    if (paint && o.final_frames != nullptr) {      // before the per-step kernel: the final frame shows the episode that ended
      rc = maze_launch_render(h, o.final_frames + k * fsz, nullptr, true);
      if (rc != XV_OK) return rc;
    }
    MzRow R;
    R.command = o.command + 3 * r; R.pos = o.pos + 2 * r; R.ori = o.ori + r; R.grid = o.grid + 2 * r;
    R.cmd_idx = o.cmd_idx + r; R.cmd_age = o.cmd_age + r; R.collision = o.collision + r; R.target = o.target + r;
    R.episode = o.episode + r; R.final_pose = o.final_pose ? o.final_pose + 3 * r : nullptr;
    R.steps_next = t + 1 < T ? o.steps + r + n : nullptr;
    rc = maze_launch_poststep(h, R, false, nullptr);
    if (rc != XV_OK) return rc;
    if (paint) {
      rc = maze_launch_render(h, o.frames + k * fsz, nullptr, false);
      if (rc != XV_OK) return rc;
    }
  }
  return XV_OK;
}

extern "C" int xv_maze_rollout(xv_maze* h, const void* actions, int action_mode, int T, int frame_stride, int autoreset_mode,
                               const xv_maze_rollout_out* out) {
  XV_CHECK_ARG(h != nullptr);
  const int rc = xv_maze_rollout_check(h->a.n_env, action_mode, autoreset_mode, T, frame_stride, actions, out, 0, 0.0);
  if (rc != XV_OK) return rc;
  return maze_rollout_steps(h, nullptr, nullptr, actions, action_mode, T, frame_stride, autoreset_mode, 0.0, *out);
}

extern "C" int xv_maze_rollout_agent(xv_maze_agent* agent, xv_maze_agent* label, int T, double epsilon, int frame_stride,
                                     const xv_maze_rollout_out* out) {
  XV_CHECK_ARG(agent != nullptr);
  xv_maze* h = maze_agent_env(agent);
  XV_CHECK_ARG(label == nullptr || (label != agent && maze_agent_env(label) == h &&
                                    maze_agent_n_actions(label) == maze_agent_n_actions(agent)));
  const int action_mode = maze_agent_n_actions(agent) == 16 ? XV_MAZE_ACTION_DISCRETE16 : XV_MAZE_ACTION_DISCRETE32;
  const int rc = xv_maze_rollout_check(h->a.n_env, action_mode, XV_AUTORESET_SAME_STEP, T, frame_stride, nullptr, out, 1, epsilon);
  if (rc != XV_OK) return rc;
  return maze_rollout_steps(h, agent, label, nullptr, action_mode, T, frame_stride, XV_AUTORESET_SAME_STEP, epsilon, *out);
}

#endif  // XV_KERNELS_ONLY
