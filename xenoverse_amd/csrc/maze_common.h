// maze_common.h — what maze.hip (move / rules / ray-cast) and maze_agent.hip (the rule-based teacher) share: the kernel
// argument block, the engine-side handle and the reference's action tables.
#pragma once
#include "philox.h"
#include "xv_common.h"

#include <type_traits>

#define MZ_PI 3.1415926     // dynamics.py:7-8, the reference's own truncated constants
#define MZ_TPI 6.2831852

struct MazeArgs {
  xv_maze_tables T;
  const int32_t* env_task;
  double* pos;       // [2][n_env]
  double* ori;
  int32_t* grid;     // [2][n_env]
  int32_t* steps;
  int32_t* cmd_idx;
  int32_t* cmd_age;
  uint8_t* need_reset;
  double* collision;
  int HC;   // rows per LDS chunk of the ray-caster
  int NSUB; // columns of that chunk (rows mapping; set per launch by maze_launch_render)
  // packed RGBX-byte copies of the texture libraries ([n][256][MZ_TEX_PITCH] uint32), nullptr if not integral
  const uint32_t* pk_walls;
  const uint32_t* pk_grounds;
  const uint32_t* pk_ceilings;
  // the same texels with PAIRS of filter rows interleaved ([n][128][MZ_TEX_PITCH][2]): what the fp32 filter fetches (round 4)
  const uint32_t* pp_walls;
  const uint32_t* pp_grounds;
  const uint32_t* pp_ceilings;
  // pose of envs that ended this step, kept for the optional final frame
  double* fin_pose;  // [3][n_env]
  int32_t* fin_cmd;  // [n_env]
  uint8_t* fin_flag; // [n_env] 1: this step's move launch reset the env (same-step: it ended; next-step: it was due)
  uint32_t* err;
  int n_env, n_task, NG, n_cmd, max_steps, W, H, command_in_observation;
  double collision_dist, visibility;
};

struct xv_maze {
  xv_engine* eng;
  MazeArgs a;
  int filter = 0;            // xv_maze_set_precision (XV_MAZE_FILTER_*)
  int raycast_mapping = 0;   // xv_maze_set_raycast_mapping (XV_MAZE_MAP_*)
  bool typing_numba = false; // xv_maze_set_typing
  bool move_lanes9 = true;   // xv_maze_set_move_kernel
  int move_lanes = 0;        // 0: by batch size; 3 or 9: forced (xv_maze_set_move_kernel)
  int move_compact = -1;     // -1: by batch size; 0 / 1: forced (xv_maze_set_move_kernel)
  int32_t* move_list = nullptr;   // [n_env] envs the nine-lane kernel has to walk this step (maze_move_sort_kernel)
  int32_t* move_count = nullptr;  // [2][2] {envs to walk, envs standing still}; the two pairs alternate between steps
  int move_word = 0;
  // resampled episodes (xv_maze_set_episode_resample; maze_rollout.hip): flags 0 = off
  int re_flags = 0;
  uint64_t re_seed = 0;
  int64_t re_index_base = 0, re_episode_base = 0;
  int32_t* re_episodes = nullptr;   // [n_env] resets of each env so far (the caller's memory)
};

// Row t of a rollout's record, every pointer already at [t][0] (all null: no record is written — the per-step kernel then
// only restarts episodes); steps_next: row t + 1 of `steps`, or null.
struct MzRow {
  float* command;
  double* pos;
  double* ori;
  int32_t* grid;
  int32_t* cmd_idx;
  int32_t* cmd_age;
  double* collision;
  int32_t* target;
  int32_t* episode;
  double* final_pose;
  int32_t* steps_next;
};
// The per-step kernel (maze_rollout.hip), one wave per env, after the move of a step: with resampled episodes on, an env
// whose fin_flag is set (the move launch reset it) gets its task resampled and is placed at the new start; then row R.
// reset_mask: instead of fin_flag, xv_maze_reset's mask semantics (null = every env) — the resampling reset itself.
int maze_launch_poststep(xv_maze* h, const MzRow& R, bool is_reset, const uint8_t* reset_mask);

// what the fused rollouts (maze_rollout.hip) issue per step: the launches of xv_maze_step and xv_maze_agent_act, one by one
int maze_launch_move(xv_maze* h, const void* action, int action_mode, float* reward, uint8_t* terminated, uint8_t* truncated,
                     int autoreset_mode);                                                    // maze.hip
int maze_launch_render(xv_maze* h, uint8_t* frames, float* command_rgb, bool final);      // maze.hip
// epsilon-greedy on top of an agent's decision, made where the decision is stored (maze_agent_kernel).  Off (the default,
// what xv_maze_agent_act passes): every pointer null.  explored (uint8[n_env]) non-null: w = xv_env_draw(seed, env id, the
// act's tick, XV_DRAW_EXPLORE); the env explores iff u53(w.x, w.y) < epsilon and then executes floor(u53(w.z, w.w) * n_actions).
// own (int32[n_env], nullable): the agent's own choice, whatever is executed.
// (The purpose byte lives here, with the family that draws it, as the other families' do beside philox.h's common ones:
// philox.h is part of the source hash that ties the committed AnyMDP counter profiles to the kernels they measured.)
#define XV_DRAW_EXPLORE 48u   // env-draw purpose: words 0,1 -> the explore coin, words 2,3 -> the random action
struct MazeExplore {
  double epsilon;
  int32_t* own;
  uint8_t* explored;
};
struct xv_maze_agent;
int maze_agent_launch(xv_maze_agent* g, const uint8_t* exposed_inject, int32_t* action, const MazeExplore& x);   // maze_agent.hip
xv_maze* maze_agent_env(xv_maze_agent* g);
int maze_agent_n_actions(xv_maze_agent* g);

static __device__ const double MZ_ACT16[16][2] = {{0.0, 0.5}, {0.05, 0.0}, {-0.05, 0.0}, {0.1, 0.0}, {-0.1, 0.0}, {0.2, 0.0},
                                           {-0.2, 0.0}, {0.3, 0.0}, {-0.3, 0.0}, {0.5, 0.0}, {-0.5, 0.0}, {0.0, 1.0},
                                           {0.05, 1.0}, {-0.05, 1.0}, {0.10, 1.0}, {-0.10, 1.0}};
static __device__ const double MZ_ACT32[32][2] = {
    {0.0, 0.2}, {0.02, 0.0}, {-0.02, 0.0}, {0.05, 0.0}, {-0.05, 0.0}, {0.1, 0.0}, {-0.1, 0.0}, {0.2, 0.0},
    {-0.2, 0.0}, {0.3, 0.0}, {-0.3, 0.0}, {0.4, 0.0}, {-0.4, 0.0}, {0.5, 0.0}, {-0.5, 0.0}, {0.0, 0.5},
    {0.0, 1.0}, {0.02, 0.5}, {0.02, 1.0}, {-0.02, 0.5}, {-0.02, 1.0}, {0.05, 0.5}, {0.05, 1.0}, {-0.05, 0.5},
    {-0.05, 1.0}, {0.10, 0.5}, {0.10, 1.0}, {-0.10, 0.5}, {-0.10, 1.0}, {0.0, -0.2}, {0.1, -0.2}, {-0.1, -0.2}};

// ray_caster_utils.py:11-25
static __device__ const float MZ_LANDMARK_RGB[XV_MAZE_LMAX][3] = {
    {0, 255, 0}, {255, 0, 0}, {0, 0, 255}, {0, 255, 255}, {255, 0, 255}, {255, 255, 0}, {128, 128, 255},
    {128, 255, 128}, {255, 128, 128}, {0, 96, 128}, {96, 0, 128}, {0, 128, 96}, {96, 128, 0}, {128, 96, 0},
    {128, 0, 96}};

__device__ __forceinline__ double mz_angle_norm(double t) {   // dynamics.py:48-54
  while (t > MZ_PI) t -= MZ_TPI;
  while (t < -MZ_PI) t += MZ_TPI;
  return t;
}

__device__ __forceinline__ void mz_reset_env(const MazeArgs& P, int e, int t) {   // maze_base.py:83-105
  const int32_t* in = P.T.ints + (size_t)t * 8;
  const double cs = P.T.dbl[(size_t)t * 8];
  const size_t N = (size_t)P.n_env;
  P.grid[e] = in[1]; P.grid[N + e] = in[2];
  P.pos[e] = in[1] * cs + 0.5 * cs;        // get_cell_center :215-218
  P.pos[N + e] = in[2] * cs + 0.5 * cs;
  P.ori[e] = 0.0;
  P.cmd_idx[e] = 0; P.cmd_age[e] = 0; P.steps[e] = 0; P.need_reset[e] = 0; P.collision[e] = 0.0;
}

__device__ __forceinline__ float xv_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double xv_abs(double v) { return fabs(v); }
__device__ __forceinline__ float xv_floor(float v) { return floorf(v); }
__device__ __forceinline__ double xv_floor(double v) { return floor(v); }
