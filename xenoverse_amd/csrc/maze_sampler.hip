// maze_sampler.hip — MazeWorld tasks made on the device: xv_maze_sample_tasks (head, rooms, Prim-style wall release,
// textures, landmarks, start, commands, written into the table slots xv_maze_create consumes) and
// xv_maze_resample_tasks (the reference's Resampler over a batch of device tables).
//
// Reference: xenoverse/mazeworld/envs/task_sampler.py (sample_task :92-177, resample_task :179-225),
// xenoverse/utils/grid_ops.py (genmaze_largeroom :49-72, genmaze_by_primwall :74-162); restated on the host in
// xenoverse_amd/mazeworld/task_sampler.py and, under this file's draws, in mazeworld/sampler_host.py, which the kernels
// are held to bit for bit.
//
// One wave64 is one workgroup is one candidate: the grid (walls, room margins / landmarks, region ids) lives in LDS,
// lane l owns cells l, l + 64, ... of the n x n grid (one cell per lane at n <= 7, ten at n = 25, 63 at n = 63), every
// choice is a cross-lane reduction whose result does not depend on how cells are dealt to lanes, and the workgroup
// barriers are those of a single wave (they order the LDS traffic, nobody waits for another wave).
//
// The wall release: nothing changes during a pass of genmaze until it breaks, so each standing wall's test (P1 joins
// regions without a loop | P2 joins regions and closes a loop, loops allowed | P3 one region left, loops allowed, its own
// uniform < 0.2) is a function of the grid as the pass found it.  With an independent key per (pass, wall), "the first
// passing wall of a shuffled order" is the passing wall with the smallest (key, cell) and "the last of the order" the
// standing wall with the largest (key, cell).  A pass = test every wall, one argmin and one argmax, release and relabel.
// The loop is bounded: 4 (n-2)^2 passes, then status pass_cap.  No loop here depends on data for its termination.
#include "xv_common.h"
#include "xv_draws.h"

namespace {

constexpr int MS_T = 64;           // one wave
constexpr int MS_N_MIN = 7, MS_N_MAX = 63;
constexpr int MS_CELLS = 64 * 64;  // LDS cells (n * n <= 3969)
constexpr int MS_CMD_MAX = 2048;
constexpr int MS_ROOM_TRIES = 5;
constexpr uint64_t MS_K53 = (1ull << 53) - 1;

// purposes (low byte of counter word 3); the resampler's are the sampler's | MS_P_RESAMPLE
enum : uint32_t { MS_P_HEAD = 0, MS_P_ROOM = 1, MS_P_PASS = 2, MS_P_TEXT = 3, MS_P_LANDMARK = 4, MS_P_START = 5, MS_P_CMD = 6,
                  MS_P_SHUFFLE = 7, MS_P_RESAMPLE = 0x10 };
enum : int { MS_OK = 0, MS_PASS_CAP = 1, MS_NO_ROOM = 2 };

struct MsLds {
  int8_t walls[MS_CELLS];     // pitch n
  int8_t mark[MS_CELLS];      // rooms' margins while rooms are dug, cell_landmarks afterwards
  uint16_t region[MS_CELLS];  // open cells: region id (lattice cell: its flat index; room q: n * n + q)
  int8_t cx[MS_CMD_MAX], cd[MS_CMD_MAX];
};

struct MsArgs {
  uint64_t seed;
  int64_t cand_base;
  int n_cand, NG;
  xv_maze_sampler_params p;
  xv_maze_task_slots o;
  xv_maze_cand_info* info;
  int32_t* status;
};

// element q of a block of uniforms: half q & 1 of call q >> 1
__device__ __forceinline__ uint64_t ms_block_k53(uint64_t seed, uint64_t index, uint32_t tick, uint32_t purpose, uint32_t q) {
  const xv_u32x4 w = xv_index_draw(seed, index, tick, purpose, q >> 1);
  return (q & 1u) ? xv_k53(w.z, w.w) : xv_k53(w.x, w.y);
}

// ---- cross-lane choices: the greatest key, equal keys to the lower index; i < 0: no entry ----
struct MsBest {
  uint64_t k;
  int i;
};
__device__ __forceinline__ bool ms_beats(const MsBest& b, const MsBest& a) {      // b replaces a
  if (b.i < 0) return false;
  if (a.i < 0) return true;
  return b.k > a.k || (b.k == a.k && b.i < a.i);
}
__device__ __forceinline__ MsBest ms_wave_best(MsBest v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MsBest w;
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v.k, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v.k >> 32), o, 64);
    w.k = ((uint64_t)hi << 32) | lo;
    w.i = __shfl_xor(v.i, o, 64);
    if (ms_beats(w, v)) v = w;
  }
  return v;
}
__device__ __forceinline__ int ms_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// a double as an integer of the same order (no NaN and no -0 reach it)
__device__ __forceinline__ uint64_t ms_ordered(double d) {
  const uint64_t b = (uint64_t)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the open neighbours of interior cell (i, j): region ids (-1 where closed; up, down, left, right), how many distinct,
// the largest multiplicity (>= 1), the smallest id (-1: none)
struct MsEval {
  int ids[4];
  int distinct, most, keep;
};
__device__ __forceinline__ MsEval ms_eval(const MsLds& L, int n, int c) {
  MsEval e;
  const int nb[4] = {c - n, c + n, c - 1, c + 1};
  e.distinct = 0; e.most = 1; e.keep = -1;
#pragma unroll
  for (int t = 0; t < 4; ++t) e.ids[t] = L.walls[nb[t]] < 1 ? (int)L.region[nb[t]] : -1;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (e.ids[t] < 0) continue;
    bool first = true;
    int same = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      same += e.ids[s] == e.ids[t];
      if (s < t && e.ids[s] == e.ids[t]) first = false;
    }
    e.distinct += first;
    e.most = same > e.most ? same : e.most;
    e.keep = (e.keep < 0 || e.ids[t] < e.keep) ? e.ids[t] : e.keep;
  }
  return e;
}

// ---- landmarks, start, commands: shared by the sampler and the resampler; the grid is in L (walls; mark = landmarks) ----
// _targets: like = u - walls; the k largest are the landmarks in ascending order of like (ties: the lower index ranks higher)
__device__ void ms_landmarks(MsLds& L, int n, uint64_t seed, uint64_t index, uint32_t tick, uint32_t purpose, int k,
                             int32_t* lm_coord) {
  const int lane = threadIdx.x, nn = n * n;
  for (int c = lane; c < nn; c += MS_T) L.mark[c] = -1;
  __syncthreads();
  for (int r = 0; r < XV_MAZE_LMAX; ++r) {
    if (r >= k) break;
    MsBest b{0, -1};
    for (int c = lane; c < nn; c += MS_T) {
      if (L.mark[c] >= 0) continue;
      const double like = xv_k53_u(ms_block_k53(seed, index, tick, purpose, (uint32_t)c)) - (double)L.walls[c];
      const MsBest v{ms_ordered(like), c};
      if (ms_beats(v, b)) b = v;
    }
    b = ms_wave_best(b);
    __syncthreads();
    if (lane == 0 && b.i >= 0) {
      const int q = k - 1 - r;
      L.mark[b.i] = (int8_t)q;
      lm_coord[2 * q] = b.i / n;
      lm_coord[2 * q + 1] = b.i % n;
    }
    __syncthreads();
  }
}
// _start: the argmax of u - walls - cell_landmarks (ties: the lower index)
__device__ int ms_start(const MsLds& L, int n, uint64_t seed, uint64_t index, uint32_t tick, uint32_t purpose) {
  const int lane = threadIdx.x, nn = n * n;
  MsBest b{0, -1};
  for (int c = lane; c < nn; c += MS_T) {
    const double like = xv_k53_u(ms_block_k53(seed, index, tick, purpose, (uint32_t)c)) - (double)L.walls[c] - (double)L.mark[c];
    const MsBest v{ms_ordered(like), c};
    if (ms_beats(v, b)) b = v;
  }
  return ms_wave_best(b).i;
}
// _sample_cmds: n_cmd draws below k, immediate repeats moved on by 1 + floor(u (k - 1)), left to right
__device__ void ms_commands(MsLds& L, uint64_t seed, uint64_t index, uint32_t tick, uint32_t purpose, int k, int n_cmd,
                            int32_t* commands) {
  const int lane = threadIdx.x;
  for (int i = lane; i < n_cmd; i += MS_T) {
    const xv_u32x4 w = xv_index_draw(seed, index, tick, purpose, (uint32_t)i);
    L.cx[i] = (int8_t)xv_floor_int(xv_u53(w.x, w.y), k);
    L.cd[i] = (int8_t)(1 + xv_floor_int(xv_u53(w.z, w.w), k - 1));
  }
  __syncthreads();
  if (lane == 0)
    for (int i = 1; i < n_cmd; ++i)
      if (L.cx[i] == L.cx[i - 1]) L.cx[i] = (int8_t)((L.cx[i] + L.cd[i]) % k);
  __syncthreads();
  for (int i = lane; i < n_cmd; i += MS_T) commands[i] = L.cx[i];
}

// ---- the sampler ----
__global__ __launch_bounds__(MS_T) void maze_sampler_kernel(MsArgs P) {
  __shared__ MsLds L;
  const int lane = threadIdx.x, ci = blockIdx.x;
  if (ci >= P.n_cand) return;
  const uint64_t cand = (uint64_t)P.cand_base + (uint64_t)ci, seed = P.seed;
  const xv_maze_sampler_params& A = P.p;
  const int NG = P.NG;

  // head
  double u[10];
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const xv_u32x4 w = xv_index_draw(seed, cand, 0, MS_P_HEAD, (uint32_t)s);
    u[2 * s] = xv_u53(w.x, w.y);
    u[2 * s + 1] = xv_u53(w.z, w.w);
  }
  const double cell_size = A.cell_size[0] + (A.cell_size[1] - A.cell_size[0]) * u[0];
  const double wall_height = A.wall_height[0] + (A.wall_height[1] - A.wall_height[0]) * u[1];
  const double agent_height = A.agent_height[0] + (A.agent_height[1] - A.agent_height[0]) * u[2];
  const double wall_density = A.wall_density[0] + (A.wall_density[1] - A.wall_density[0]) * u[3];
  int k = A.landmarks_lo + xv_floor_int(u[4], A.landmarks_hi - A.landmarks_lo);
  k = k > XV_MAZE_LMAX ? XV_MAZE_LMAX : k;
  int n = A.n_lo + xv_floor_int(u[5], A.n_hi - A.n_lo);
  n |= 1;
  n = n > NG ? NG : n;      // cannot happen with the arguments xv_maze_sample_tasks admits: the LDS grid's bound
  const int ground_text = xv_floor_int(u[6], A.n_ground_textures), ceiling_text = xv_floor_int(u[7], A.n_ceiling_textures);
  const double fol_angle = A.fol_angle[0] + (A.fol_angle[1] - A.fol_angle[0]) * u[8];
  const int m = n - 2, nn = n * n;
  const int n_rooms = xv_floor_int(u[9], m * m / 16);

  // rooms (_dig_rooms): walls all standing, margins empty
  for (int c = lane; c < nn; c += MS_T) {
    L.walls[c] = 1;
    L.mark[c] = 0;
    L.region[c] = 0;
  }
  __syncthreads();
  int rooms = 0;
  for (int r = 0; r < n_rooms; ++r) {
    for (int t = 0; t < MS_ROOM_TRIES; ++t) {
      const uint32_t sub = 2u * (uint32_t)(MS_ROOM_TRIES * r + t);
      const xv_u32x4 w0 = xv_index_draw(seed, cand, 0, MS_P_ROOM, sub),
                     w1 = xv_index_draw(seed, cand, 0, MS_P_ROOM, sub + 1);
      const int h = 2 + xv_floor_int(xv_u53(w0.x, w0.y), 3), w = 2 + xv_floor_int(xv_u53(w0.z, w0.w), 3);
      const double uk = xv_u53(w1.x, w1.y);
      const int cols = m - w + 1, places = (m - h + 1) * cols;
      // free placements, 64 at a time in row-major order: ballots count them and find the k-th
      int n_free = 0;
      for (int base = 0; base < places; base += MS_T) {
        const int p = base + lane;
        bool fr = p < places;
        if (fr) {
          const int r0 = p / cols, c0 = p - r0 * cols;
          for (int a = 0; a < h; ++a)
            for (int b = 0; b < w; ++b) fr = fr && L.mark[(r0 + 1 + a) * n + c0 + 1 + b] == 0;
        }
        n_free += __popcll(__ballot(fr));
      }
      if (n_free == 0) continue;
      const int pick = xv_floor_int(uk, n_free);
      int seen = 0, place = -1;
      for (int base = 0; base < places; base += MS_T) {
        const int p = base + lane;
        bool fr = p < places;
        if (fr) {
          const int r0 = p / cols, c0 = p - r0 * cols;
          for (int a = 0; a < h; ++a)
            for (int b = 0; b < w; ++b) fr = fr && L.mark[(r0 + 1 + a) * n + c0 + 1 + b] == 0;
        }
        const uint64_t bal = __ballot(fr);
        const int cnt = __popcll(bal);
        if (place < 0 && pick < seen + cnt) {      // the (pick - seen)-th set bit of the ballot
          uint64_t bits = bal;
          for (int s = 0; s < MS_T; ++s) {
            if (s >= pick - seen) break;
            bits &= bits - 1;
          }
          place = base + (int)__builtin_ctzll(bits);
        }
        seen += cnt;
      }
      __syncthreads();
      // the room and its one-cell margin (clipped to the interior): up to 6 x 6 cells, one per lane
      const int r0 = place / cols, c0 = place - r0 * cols;
      if (place >= 0 && lane < 36) {
        const int di = lane / 6, dj = lane - 6 * di;
        const int ri = r0 - 1 + di, cj = c0 - 1 + dj;      // interior coordinates
        if (di < h + 2 && dj < w + 2 && ri >= 0 && ri < m && cj >= 0 && cj < m) {
          const int c = (ri + 1) * n + cj + 1;
          L.mark[c] = 1;
          if (di >= 1 && di <= h && dj >= 1 && dj <= w) {
            L.walls[c] = 0;
            L.region[c] = (uint16_t)(nn + rooms);
          }
        }
      }
      __syncthreads();
      ++rooms;
      break;
    }
  }

  // regions: every odd-lattice cell outside the margins is its own region, every room is one
  int n_lattice = 0, n_walls = 0;
  for (int c = lane; c < nn; c += MS_T) {
    const int i = c / n, j = c - i * n;
    const bool inner = i >= 1 && i <= n - 2 && j >= 1 && j <= n - 2;
    if (inner && (i & 1) && (j & 1) && L.mark[c] == 0) {
      L.walls[c] = 0;
      L.region[c] = (uint16_t)c;
      ++n_lattice;
    }
    n_walls += inner && L.walls[c] != 0;
  }
  __syncthreads();
  int n_regions = ms_wave_sum(n_lattice) + rooms;
  n_walls = ms_wave_sum(n_walls);

  // passes
  const bool loops = A.allow_loops != 0;
  const double budget = (double)(m * m) * wall_density;
  const int cap = 4 * m * m;
  int passes = 0, idle = 0, released = 0;
  for (; passes < cap; ++passes) {
    if (!(n_regions > 1 || (loops && (double)n_walls > budget))) break;
    MsBest first{0, -1}, last{0, -1};
    for (int c = lane; c < nn; c += MS_T) {
      const int i = c / n, j = c - i * n;
      if (i < 1 || i > n - 2 || j < 1 || j > n - 2 || L.walls[c] == 0) continue;
      const MsEval e = ms_eval(L, n, c);
      const xv_u32x4 w = xv_index_draw(seed, cand, (uint32_t)passes, MS_P_PASS, (uint32_t)c);
      const uint64_t key = xv_k53(w.x, w.y);
      const bool pass = (e.distinct >= 2 && (e.most < 2 || loops)) || (loops && n_regions < 2 && xv_u53(w.z, w.w) < 0.2);
      const MsBest lo{MS_K53 - key, c}, hi{key, MS_CELLS - 1 - c};      // smallest (key, cell); largest (key, cell)
      if (pass && ms_beats(lo, first)) first = lo;
      if (ms_beats(hi, last)) last = hi;
    }
    first = ms_wave_best(first);
    last = ms_wave_best(last);
    const int chosen = first.i >= 0 ? first.i : (last.i >= 0 ? MS_CELLS - 1 - last.i : -1);
    if (chosen < 0) {
      ++idle;
      continue;
    }
    const MsEval e = ms_eval(L, n, chosen);      // every lane, the same cell
    if (e.keep < 0) {      // the wall the pass ended on touches no open cell
      ++idle;
      continue;
    }
    __syncthreads();
    if (lane == 0) {
      L.walls[chosen] = 0;
      L.region[chosen] = (uint16_t)e.keep;
    }
    if (e.distinct > 1)
      for (int c = lane; c < nn; c += MS_T) {
        if (c == chosen || L.walls[c] != 0) continue;
        const int rid = L.region[c];
        if (rid != e.keep && (rid == e.ids[0] || rid == e.ids[1] || rid == e.ids[2] || rid == e.ids[3]))
          L.region[c] = (uint16_t)e.keep;
      }
    __syncthreads();
    --n_walls;
    ++released;
    n_regions -= e.distinct - 1;
  }
  int status = (n_regions > 1 || (loops && (double)n_walls > budget)) ? MS_PASS_CAP : MS_OK;
  if (status == MS_OK && m * m - n_walls < k + 1) status = MS_NO_ROOM;

  const size_t slot = (size_t)ci * NG * NG;
  int32_t* ints = P.o.ints + (size_t)ci * 8;
  double* dbl = P.o.dbl + (size_t)ci * 8;
  int32_t* commands = P.o.commands + (size_t)ci * A.n_cmd;
  int32_t* lm_coord = P.o.lm_coord + (size_t)ci * XV_MAZE_LMAX * 2;
  int start = 0;
  if (status == MS_OK) {
    ms_landmarks(L, n, seed, cand, 0, MS_P_LANDMARK, k, lm_coord);
    start = ms_start(L, n, seed, cand, 0, MS_P_START);
    ms_commands(L, seed, cand, 0, MS_P_CMD, k, A.n_cmd, commands);
  } else {
    for (int i = lane; i < A.n_cmd; i += MS_T) commands[i] = 0;
  }
  if (lane < 2 * XV_MAZE_LMAX && (status != MS_OK || lane >= 2 * k)) lm_coord[lane] = 0;      // every word written once
  // the slots, padded: walls 1, texts 0, landmarks -1 (a candidate without a table is all padding)
  for (int p = lane; p < NG * NG; p += MS_T) {
    const int i = p / NG, j = p - i * NG;
    int8_t wv = 1, lv = -1;
    int32_t tv = 0;
    if (status == MS_OK && i < n && j < n) {
      const int c = i * n + j;
      wv = L.walls[c];
      lv = L.mark[c];
      const bool inner = i >= 1 && i <= n - 2 && j >= 1 && j <= n - 2;
      if (!(inner && wv < 1))
        tv = xv_floor_int(xv_k53_u(ms_block_k53(seed, cand, 0, MS_P_TEXT, (uint32_t)c)), A.n_wall_textures);
    }
    P.o.walls[slot + p] = wv;
    P.o.texts[slot + p] = tv;
    P.o.landmarks[slot + p] = lv;
  }
  if (lane == 0) {
    for (int q = 0; q < 8; ++q) {
      if (status != MS_OK || q >= 6) ints[q] = 0;
      if (status != MS_OK || q >= 7) dbl[q] = 0.0;
    }
    if (status == MS_OK) {
      ints[0] = n; ints[1] = start / n; ints[2] = start % n; ints[3] = ground_text; ints[4] = ceiling_text; ints[5] = k;
      dbl[0] = cell_size; dbl[1] = wall_height; dbl[2] = agent_height; dbl[3] = fol_angle; dbl[4] = A.step_reward;
      dbl[5] = A.has_goal_reward ? A.goal_reward : (double)n * sqrt((double)n) / 60.0;
      dbl[6] = A.collision_reward;      // dbl[7] = tan(fol_angle / 2) is the host's (numpy.tan): left 0 here
    }
    P.status[ci] = status;
    if (P.info) P.info[ci] = xv_maze_cand_info{status, n, rooms, passes, idle, released};
  }
}

// ---- the resampler: one wave per task, in place on landmarks / lm_coord / ints[1:3] / commands ----
struct MsReArgs {
  uint64_t seed;
  int64_t index_base;
  uint32_t episode;
  int n_task, NG, n_cmd, flags;
  xv_maze_task_slots o;
};

// The Resampler on task slot `ti` of P.o for one wave (every lane of it calls this; L is the wave's own): the draws are a
// function of (P.seed, P.index_base + ti, episode).  Shared by maze_resampler_kernel (one episode for every task) and
// the per-step kernel of the fused rollouts (maze_rollout.hip: the episode is the env's own reset count).
__device__ void ms_resample_task(MsLds& L, const MsReArgs& P, int ti, uint32_t episode) {
  const int lane = threadIdx.x;
  const int NG = P.NG;
  int32_t* ints = P.o.ints + (size_t)ti * 8;
  const int n = ints[0], k = ints[5];
  if (n < 3 || n > NG || n > MS_N_MAX || k < 1 || k > XV_MAZE_LMAX) return;      // not a task of this engine: untouched
  const uint64_t index = (uint64_t)P.index_base + (uint64_t)ti, seed = P.seed;
  const size_t slot = (size_t)ti * NG * NG;
  int32_t* lm_coord = P.o.lm_coord + (size_t)ti * XV_MAZE_LMAX * 2;
  const int nn = n * n;
  for (int c = lane; c < nn; c += MS_T) {
    const int i = c / n, j = c - i * n;
    L.walls[c] = P.o.walls[slot + (size_t)i * NG + j];
    L.mark[c] = P.o.landmarks[slot + (size_t)i * NG + j];
  }
  __syncthreads();
  if (P.flags & XV_MAZE_RESAMPLE_LANDMARKS) {
    ms_landmarks(L, n, seed, index, episode, MS_P_LANDMARK | MS_P_RESAMPLE, k, lm_coord);
  } else if (P.flags & XV_MAZE_RESAMPLE_COLOR) {
    // a random permutation by key rank: the new landmark r is the old landmark with the r-th smallest (key, id)
    const uint64_t key = lane < k ? ms_block_k53(seed, index, episode, MS_P_SHUFFLE | MS_P_RESAMPLE, (uint32_t)lane) : 0;
    int ci = 0, cj = 0, rank = 0;
    if (lane < k) {
      ci = lm_coord[2 * lane];
      cj = lm_coord[2 * lane + 1];
    }
    for (int q = 0; q < XV_MAZE_LMAX; ++q) {
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)key, q, 64), hi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), q, 64);
      const uint64_t kq = ((uint64_t)hi << 32) | lo;
      if (q < k && (kq < key || (kq == key && q < lane))) ++rank;
    }
    __syncthreads();
    if (lane < k && ci >= 0 && ci < n && cj >= 0 && cj < n) {
      lm_coord[2 * rank] = ci;
      lm_coord[2 * rank + 1] = cj;
      L.mark[ci * n + cj] = (int8_t)rank;
    }
    __syncthreads();
  }
  if (P.flags & XV_MAZE_RESAMPLE_START) {
    const int start = ms_start(L, n, seed, index, episode, MS_P_START | MS_P_RESAMPLE);
    if (lane == 0 && start >= 0) {
      ints[1] = start / n;
      ints[2] = start % n;
    }
  }
  if (P.flags & XV_MAZE_RESAMPLE_CMD)
    ms_commands(L, seed, index, episode, MS_P_CMD | MS_P_RESAMPLE, k, P.n_cmd, P.o.commands + (size_t)ti * P.n_cmd);
  if (P.flags & (XV_MAZE_RESAMPLE_LANDMARKS | XV_MAZE_RESAMPLE_COLOR))
    for (int c = lane; c < nn; c += MS_T) {
      const int i = c / n, j = c - i * n;
      P.o.landmarks[slot + (size_t)i * NG + j] = L.mark[c];
    }
}

__global__ __launch_bounds__(MS_T) void maze_resampler_kernel(MsReArgs P) {
  __shared__ MsLds L;
  if ((int)blockIdx.x >= P.n_task) return;
  ms_resample_task(L, P, (int)blockIdx.x, P.episode);
}

}  // namespace

#ifndef XV_KERNELS_ONLY

static bool ms_range_ok(const double r[2]) { return r[0] == r[0] && r[1] == r[1] && r[0] <= r[1]; }

// the argument checks of xv_maze_sample_tasks: everything before the launch, no device needed
extern "C" int xv_maze_sampler_check(int64_t cand_base, int n_cand, int NG, const xv_maze_sampler_params* p,
                                     const xv_maze_task_slots* out, const int32_t* status) {
  XV_CHECK_ARG(p != nullptr && out != nullptr && status != nullptr);
  XV_CHECK_ARG(n_cand > 0 && cand_base >= 0);
  XV_CHECK_ARG(p->n_lo >= MS_N_MIN && p->n_lo < p->n_hi && p->n_hi <= MS_N_MAX + 1);
  XV_CHECK_ARG((NG & 1) == 1 && NG >= MS_N_MIN && NG <= MS_N_MAX);
  XV_CHECK_ARG(NG == ((p->n_hi - 1) | 1));      // the largest n the range can give
  XV_CHECK_ARG(p->landmarks_lo >= 2 && p->landmarks_lo < p->landmarks_hi);
  XV_CHECK_ARG(p->n_cmd >= 1 && p->n_cmd <= MS_CMD_MAX);
  XV_CHECK_ARG(p->n_wall_textures >= 1 && p->n_ground_textures >= 1 && p->n_ceiling_textures >= 1);
  XV_CHECK_ARG(ms_range_ok(p->cell_size) && ms_range_ok(p->wall_height) && ms_range_ok(p->agent_height) &&
               ms_range_ok(p->wall_density) && ms_range_ok(p->fol_angle));
  XV_CHECK_ARG(p->agent_height[0] > 0 && p->agent_height[1] <= p->wall_height[0]);      // MazeBase.set_task's assert
  XV_CHECK_ARG(p->step_reward == p->step_reward && p->collision_reward == p->collision_reward);
  XV_CHECK_ARG(!p->has_goal_reward || p->goal_reward > 0);
  XV_CHECK_ARG(out->walls && out->texts && out->landmarks && out->ints && out->dbl && out->commands && out->lm_coord);
  return XV_OK;
}

extern "C" int xv_maze_sample_tasks(xv_engine* e, uint64_t seed, int64_t cand_base, int n_cand, int NG,
                                    const xv_maze_sampler_params* p, const xv_maze_task_slots* out, xv_maze_cand_info* info,
                                    int32_t* status) {
  XV_CHECK_ARG(e != nullptr);
  const int rc = xv_maze_sampler_check(cand_base, n_cand, NG, p, out, status);
  if (rc != XV_OK) return rc;
  XV_HIP(hipSetDevice(e->device));
  MsArgs P{};
  P.seed = seed; P.cand_base = cand_base; P.n_cand = n_cand; P.NG = NG; P.p = *p; P.o = *out; P.info = info; P.status = status;
  hipLaunchKernelGGL(maze_sampler_kernel, dim3(n_cand), dim3(MS_T), 0, e->stream, P);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_maze_resample_tasks(xv_engine* e, uint64_t seed, int64_t index_base, int64_t episode, int n_task, int NG,
                                      int n_cmd, int flags, const xv_maze_task_slots* io) {
  XV_CHECK_ARG(e != nullptr && io != nullptr);
  XV_CHECK_ARG(n_task > 0 && index_base >= 0 && episode >= 0 && episode < ((int64_t)1 << 24));
  XV_CHECK_ARG(NG >= 3 && NG <= MS_N_MAX + 1 && n_cmd >= 1 && n_cmd <= MS_CMD_MAX);
  XV_CHECK_ARG((flags & ~(XV_MAZE_RESAMPLE_CMD | XV_MAZE_RESAMPLE_START | XV_MAZE_RESAMPLE_LANDMARKS | XV_MAZE_RESAMPLE_COLOR)) == 0);
  XV_CHECK_ARG(io->walls && io->landmarks && io->ints && io->commands && io->lm_coord);
  XV_HIP(hipSetDevice(e->device));
  MsReArgs P{};
  P.seed = seed; P.index_base = index_base; P.episode = (uint32_t)episode; P.n_task = n_task; P.NG = NG; P.n_cmd = n_cmd;
  P.flags = flags; P.o = *io;
  hipLaunchKernelGGL(maze_resampler_kernel, dim3(n_task), dim3(MS_T), 0, e->stream, P);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

#endif  // XV_KERNELS_ONLY
