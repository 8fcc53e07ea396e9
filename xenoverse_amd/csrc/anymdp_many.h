// anymdp_many.h — the host side of the AnyMDP step_many family: xv_anymdp_step_many with its cached cycle graph,
// xv_anymdp_step_many_chains (views as streams or as the branches of one graph), the overlapped path of the MDP and the token
// steps with its replay, and xv_anymdp_step_tokens_many.  Host code only; anymdp.hip includes it at the end of its
// `#ifndef XV_KERNELS_ONLY` block, after everything used here (kernels, handle, lanes, variant selectors, the single-step
// launchers, anymdp_io / anymdp_tok_io, the token host code).  Each thing is here once:
//   AnyMDPRings / AnyMDPTokRings   the ring buffers of a call; slot(j) is THE way from a ring slot to the kernels' IO struct
//   anymdp_key_same / _store       a graph's key — filled whole into a zeroed local, compared whole, stored whole
//   anymdp_many_prepare / _cycle   graph + tick word, one replayed ring cycle: the handle's own graph and the parent's chain graph
//   anymdp_pipe_call               the overlapped call, MDP and token steps alike (what differs comes in as callables and values)
#pragma once

// the rings of a step_many call: slot j of each starts j * stride elements in (stride: n_env for the handle's own rings; the
// parent's n_env when a view steps its columns of the parent's rings, xv_anymdp_step_many_chains)
struct AnyMDPRings {
  size_t stride;
  const int32_t* actions; int32_t* obs; float* reward; float* reward_gt; uint8_t* terminated; uint8_t* truncated; int32_t* final_obs;
  AnyMDPStepIO slot(int j) const {
    const size_t o = (size_t)j * stride;
    return anymdp_io(actions + o, obs + o, reward + o, reward_gt + o, terminated + o, truncated + o, final_obs ? final_obs + o : nullptr);
  }
  AnyMDPRings shifted(size_t lo) const {      // the rings of a view's columns [lo, ...)
    return AnyMDPRings{stride, actions + lo, obs + lo, reward + lo, reward_gt + lo, terminated + lo, truncated + lo,
                       final_obs ? final_obs + lo : nullptr};
  }
};

// the rings of a step_tokens_many call: slot j of actions starts j * n_env * d_act elements in, of obs / final_obs
// j * n_env * d_obs, of the others j * n_env
struct AnyMDPTokRings {
  const int32_t* actions; int32_t* obs; float* reward; float* reward_gt; uint8_t* terminated; uint8_t* truncated; int32_t* final_obs;
  AnyMDPTokIO slot(const xv_anymdp* h, int j) const {
    const size_t o = (size_t)j * (size_t)h->a.n_env, da = (size_t)h->d_act, dob = (size_t)h->d_obs;
    return anymdp_tok_io(actions + o * da, obs + o * dob, reward + o, reward_gt + o, terminated + o, truncated + o,
                         final_obs ? final_obs + o * dob : nullptr);
  }
};

// A graph's key (graph_key, pipe_key, tpipe_key, cgraph_key of the handle) says what is baked into the kernel nodes' arguments.
// The caller memsets a local key to zero — the structs have padding —, fills EVERY field in one place and hands it to these two:
// current means the whole key equals the stored one; a rebuilt graph's key is stored whole.  (A zeroed key equals no filled one.)
template <class R> static void anymdp_ring_pointers(const R& r, const void** p) {      // of either ring type, as a key lists them
  p[0] = r.actions; p[1] = r.obs; p[2] = r.reward; p[3] = r.reward_gt; p[4] = r.terminated; p[5] = r.truncated; p[6] = r.final_obs;
}
template <class K> static bool anymdp_key_same(const K& want, const K& have) { return memcmp(&want, &have, sizeof(K)) == 0; }
template <class K> static void anymdp_key_store(K* have, const K& want) { memcpy(have, &want, sizeof(K)); }

// One ring cycle of xv_anymdp_step_many as a graph: `period` step-kernel nodes in a chain (node j reads actions slot j,
// writes output slot j, draws with tick *d_tick + j) and a node that advances *d_tick by `period`.  Back-to-back
// dependent launches cost ~3.3 us each on a stream and ~1.6 us as graph nodes (scripts/devtools/graph_floor.hip).
static void* anymdp_graph_step_fn(const xv_anymdp* h, int eff, int mode, bool hand = false) {
  // the hand-off (HAND) kernels exist for the fence and bucket searches only: nullptr for the binary search
  return anymdp_select_variant(anymdp_variant_g(h, eff), anymdp_variant_bk(h, eff), mode, [&](auto v) -> void* {
    using V = decltype(v);
    if constexpr (V::g != 0)
      if (hand) return reinterpret_cast<void*>(&anymdp_step_kernel<false, V::g, false, true, V::bk, true, V::md>);
    return hand ? nullptr : reinterpret_cast<void*>(&anymdp_step_kernel<false, V::g, false, true, V::bk, false, V::md>);
  });
}

// One step node of a graph: launch tick *d_tick + g, ring slot j.  The struct holds the kernel's arguments, which must live
// until hipGraphAddKernelNode has taken them.
struct AnyMDPStepNode {
  AnyMDPArgs a;
  AnyMDPStepIO io;
  int T, md;
  void* params[4];
  void fill(hipKernelNodeParams* np, const xv_anymdp* h, void* fn, uint64_t* d_tick, int g, int j, const AnyMDPRings& R, int mode) {
    a = h->a;
    a.seed = h->eng->seed; a.gid_base = h->eng->env_id_base;
    a.tick = (uint64_t)g; a.tick_dev = d_tick;
    io = R.slot(j);
    T = 1; md = mode;
    params[0] = &a; params[1] = &io; params[2] = &T; params[3] = &md;
    np->func = fn; np->gridDim = dim3(xv_div_up(h->a.n_env, 256)); np->blockDim = dim3(256); np->kernelParams = params;
  }
};

// the chain of `period` step nodes of handle `h` appended to `graph` behind `prev` (nullptr: a root); -> its last node
static bool anymdp_add_chain(xv_anymdp* h, hipGraph_t graph, hipGraphNode_t* prev, uint64_t* d_tick, int eff, int period,
                             const AnyMDPRings& R, int mode) {
  void* fn = anymdp_graph_step_fn(h, eff, mode);
  for (int j = 0; j < period; ++j) {
    hipKernelNodeParams np;
    memset(&np, 0, sizeof(np));
    AnyMDPStepNode sn;
    sn.fill(&np, h, fn, d_tick, j, j, R, mode);
    hipGraphNode_t node;
    if (hipGraphAddKernelNode(&node, graph, *prev ? prev : nullptr, *prev ? 1 : 0, &np) != hipSuccess) return false;
    *prev = node;
  }
  return true;
}

static bool anymdp_add_tick_node(hipGraph_t graph, const hipGraphNode_t* deps, int n_deps, uint64_t* d_tick, int period) {
  hipKernelNodeParams np;
  memset(&np, 0, sizeof(np));
  uint64_t dv = (uint64_t)period;
  void* tick_params[] = {&d_tick, &dv};
  np.func = reinterpret_cast<void*>(&anymdp_advance_tick_kernel); np.gridDim = dim3(1); np.blockDim = dim3(1);
  np.kernelParams = tick_params;
  hipGraphNode_t node;
  return hipGraphAddKernelNode(&node, graph, deps, (size_t)n_deps, &np) == hipSuccess;
}

static bool anymdp_ensure_graph(xv_anymdp* h, int period, const AnyMDPRings& R, int mode) {
  const int eff = anymdp_effective_search(h);
  decltype(h->graph_key) want;
  memset(&want, 0, sizeof want);
  want.period = period; want.mode = mode; want.search = eff; want.fast = (int)(eff != XV_ANYMDP_SEARCH_BINARY); want.nbk = h->a.NBK;
  want.seed = h->eng->seed; want.gid_base = h->eng->env_id_base; want.stride = R.stride;
  anymdp_ring_pointers(R, want.ptrs);
  want.bucket = (const void*)h->a.bucket;
  if (h->graph_exec && anymdp_key_same(want, h->graph_key)) return true;
  anymdp_drop_graph(h);
  if (!h->d_tick && hipMalloc(&h->d_tick, sizeof(uint64_t)) != hipSuccess) return false;
  if (hipGraphCreate(&h->graph, 0) != hipSuccess) return false;
  hipGraphNode_t prev = nullptr;
  if (!anymdp_add_chain(h, h->graph, &prev, h->d_tick, eff, period, R, mode)) return false;
  if (!anymdp_add_tick_node(h->graph, &prev, 1, h->d_tick, period)) return false;
  if (hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0) != hipSuccess) { h->graph_exec = nullptr; return false; }
  anymdp_key_store(&h->graph_key, want);
  return true;
}

// measured (scripts/devtools/graph_step_many.py, config 2b): graph replay wins 7-9 % at 1,024-4,096 envs, nothing at
// 16,384 and loses 2-3 % at 65,536 in config 2a when thousands of steps are issued (its kernels read the tick from memory;
// the stream is not the limiter) — but a SHORT burst is one submission instead of n_steps: 20 steps of 65,536 envs take
// 154 instead of 173 us.  AUTO: small batches, or short bursts.
#define XV_ANYMDP_GRAPH_AUTO_MAX 8192
#define XV_ANYMDP_GRAPH_AUTO_STEPS 128
static inline bool anymdp_graph_wanted(const xv_anymdp* h, int n_steps) {
  if (h->eng->dev_tick) return false;   // the graph keeps its own tick word, fed from the host tick: plain launches here
  return h->graph_mode == 1 ||
         (h->graph_mode == 2 && (h->a.n_env <= XV_ANYMDP_GRAPH_AUTO_MAX || n_steps <= XV_ANYMDP_GRAPH_AUTO_STEPS));
}

extern "C" int xv_anymdp_set_step_many_graph(xv_anymdp* h, int mode) {
  XV_CHECK_ARG(h != nullptr && mode >= 0 && mode <= 2);
  h->graph_mode = mode;
  return XV_OK;
}

extern "C" int xv_anymdp_step_many_graph_state(xv_anymdp* h) {   // 0 plain launches, 1 graph built and in use, -1 failed
  if (!h) return 0;
  if (h->graph_failed) return -1;
  return (h->graph_mode != 0 && (h->graph_exec || h->cgraph_exec) && h->graph_used_last) ? 1 : 0;
}

// The stepping of xv_anymdp_step_many in three pieces, so that xv_anymdp_step_many_chains can interleave the cycles of
// several handles and replay the parent's chain graph with the same code: prepare (a graph + the handle's tick word), one ring
// cycle, one plain step.  `sticky`: a failure turns the graphs off on this handle for good (graph_failed: same kernels, plain
// launches, never retried); the parent's chain graph is tried again by the next call instead.
static void anymdp_many_failed(xv_anymdp* h, bool sticky) {
  (void)hipGetLastError();
  if (sticky) h->graph_failed = true;
  h->d_tick_valid = false;
}

// `wanted`: the caller's own conditions for a graph; ensure(): the graph the cycles will replay, built or reused
template <class Ensure>
static bool anymdp_many_prepare(xv_anymdp* h, int n_steps, int period, bool wanted, bool sticky, Ensure&& ensure) {
  h->graph_used_last = false;
  if (n_steps / period <= 0 || period <= 1 || h->graph_failed || !wanted) return false;
  bool ok = ensure();
  if (ok && !(h->d_tick_valid && h->d_tick_value == h->eng->tick)) {      // bring *d_tick to the engine's tick
    hipLaunchKernelGGL(anymdp_set_tick_kernel, dim3(1), dim3(1), 0, h->eng->stream, h->d_tick, h->eng->tick);
    ok = hipGetLastError() == hipSuccess;
    if (ok) { h->d_tick_value = h->eng->tick; h->d_tick_valid = true; }
  }
  if (!ok) anymdp_many_failed(h, sticky);
  return ok;
}

// one ring cycle: `exec` replayed on the handle's stream and booked on the handle (engine tick, what *d_tick then holds)
static bool anymdp_many_cycle(xv_anymdp* h, hipGraphExec_t exec, int period, bool sticky) {
  if (hipGraphLaunch(exec, h->eng->stream) != hipSuccess) {
    anymdp_many_failed(h, sticky);
    return false;
  }
  h->eng->tick += (uint64_t)period;
  h->d_tick_value = h->eng->tick;
  h->d_tick_valid = true;
  h->graph_used_last = true;
  return true;
}

static int anymdp_many_plain(xv_anymdp* h, int k, int period, const AnyMDPRings& R, int mode) {
  anymdp_bind_rng(h, 1);
  return anymdp_launch_step<false>(h, R.slot(k % period), 1, mode);
}

// Overlapped step_many: consecutive vector steps alternate between the engine's stream (even steps) and a side stream (odd
// steps) with NO dependency between the streams — step k + 1 is dispatched while step k runs, and each of its waves takes
// its envs over from the same wave of step k through the hand-off word (HAND kernels, anymdp.hip).  What a stream's barrier
// between two launches costs — the drain of one launch and the dispatch of the next, 2.7 of the step's 5.0 us at 65,536
// envs — is then covered by the other stream's launch.  Whole ring cycles of an even period replay two cycle graphs (ring
// slots 0, 2, ... / 1, 3, ..., each with its own tick word advanced by its own last node); what is left over runs the ordinary
// way behind the join.  Calls shorter than XV_ANYMDP_PIPE_GRAPH_MIN steps take the ordinary path altogether: the second
// hipGraphLaunch reaches the device ~12-25 us after the first and the join costs a cross-queue wait, so a 20-step burst
// (~110 us) loses what the overlap gains (measured 5.9-6.4 vs 5.55 us per step; issuing the steps as plain launches
// alternately on the two streams is host-bound: 5.7; both chains as the branches of ONE graph: 6.8, and 4.3 instead of 3.7
// on long calls; profiles/r05_c_*, r05_d_burst_timeline.txt, r05_n_*).  Same launch ticks, same
// results as the ordinary path (tests/test_gpu_chains.py).
#define XV_ANYMDP_PIPE_GRAPH_MIN 64      // calls of at least this many steps are overlapped
// the side streams of *D lanes (fewer where no third stream qualifies: *D = 2 then) and what is this handle's own: the graphs'
// tick words, the gate, the snapshot for the replay
static bool anymdp_pipe_setup(xv_anymdp* h, int* D) {
  const XvPipeLanes L = anymdp_pipe_lanes(h, false);
  if (xv_pipe_streams_stale(L)) anymdp_pipe_drop_graphs(h);      // the engine moved to another stream: choose again
  const int got = xv_pipe_ensure_streams(L, *D);
  if (got == 0) return false;
  if (got < *D) (void)hipGetLastError();      // no third stream qualifies: two
  *D = got;
  if (!h->d_ptick && hipMalloc(&h->d_ptick, XV_PIPE_DEPTH_MAX * sizeof(uint64_t)) != hipSuccess) return false;   // the graphs' tick words
  if (!h->gate.d_seen && !xv_pipe_gate_create(&h->gate)) return false;
  if (!h->d_snap && hipMalloc(&h->d_snap, (size_t)h->a.n_env * sizeof(uint2)) != hipSuccess) { h->d_snap = nullptr; return false; }
  if (!h->d_snap_w) {
    if (hipMalloc(&h->d_snap_w, 4 * sizeof(uint32_t)) != hipSuccess) { h->d_snap_w = nullptr; return false; }
    if (hipMemsetAsync(h->d_snap_w, 0, 4 * sizeof(uint32_t), h->eng->stream) != hipSuccess) return false;
  }
  return true;
}
// the replay kernel for this handle's layout and search (HAND kernels exist for the fence and bucket searches only); the token
// steps' is anymdp_tok_launch_replay (anymdp.hip)
static bool anymdp_launch_replay(xv_anymdp* h, int eff, const AnyMDPStepIO& io, int period, int cycles, int mode, uint64_t t0) {
  AnyMDPArgs a = h->a;
  a.seed = h->eng->seed; a.gid_base = h->eng->env_id_base; a.tick = t0; a.tick_dev = nullptr;
  const dim3 grid(xv_div_up(h->a.n_env, 256)), block(256);
  uint32_t* h_fell = h->gate.d_issued + 1;
  anymdp_select_variant(h->a.G, anymdp_variant_bk(h, eff), -1, [&](auto v) {
    using V = decltype(v);
    if constexpr (V::g != 0)
      hipLaunchKernelGGL((anymdp_replay_kernel<V::g, V::bk>), grid, block, 0, h->eng->stream, a, io, period, cycles, mode,
                         (const uint2*)h->d_snap, h->d_snap_w, h->a.err, h_fell);
  });
  return hipGetLastError() == hipSuccess;
}

// One of the handle's two graph sets on D lanes — the MDP steps' or the token steps' (at most one is built at a time) —, current
// when `want` equals the stored key; node(g, slot, q, np) fills the kernel-node parameters of step g on lane q
// -> cycles per graph the call uses (graphs built / reused), 0: this call is not overlapped, -1: failure (or !buildable)
template <class K, class Node>
static int anymdp_pipe_graph_set(xv_anymdp* h, bool tokens, int D, int period, int cycles, const K& want, K* key, Node&& node,
                                 bool buildable = true) {
  const hipGraphExec_t* exec = tokens ? h->tgraph_exec : h->pgraph_exec;
  const bool same = exec[0] && exec[1] && anymdp_key_same(want, *key);
  const int have = (same && h->gate.depth == D) ? h->gate.unroll[tokens] : 0;
  const int U = xv_pipe_pick_unroll(period, cycles, have, D);
  if (U == 0 || U == have) return U;
  anymdp_pipe_drop_graphs(h);      // (the other set goes with it)
  if (!buildable || !xv_pipe_build_set(anymdp_pipe_lanes(h, tokens, D), &h->gate, U, period, reinterpret_cast<void*>(&anymdp_pipe_head_kernel),
                                       h->d_ptick, h->a.err, node))
    return -1;
  h->gate.depth = D;
  anymdp_key_store(key, want);
  h->gate.unroll[tokens] = U;
  return U;
}

// the graph set of the MDP steps: HAND step kernels (none for the binary search), each lane's tick word advanced by its head node
static int anymdp_pipe_graphs(xv_anymdp* h, int D, int period, int cycles, const AnyMDPRings& R, int mode) {
  const int eff = anymdp_effective_search(h);
  decltype(h->pipe_key) want;
  memset(&want, 0, sizeof want);
  want.period = period; want.mode = mode; want.search = eff; want.stride = R.stride;
  anymdp_ring_pointers(R, want.ptrs);
  want.bucket = (const void*)h->a.bucket; want.seed = h->eng->seed; want.gid_base = h->eng->env_id_base;
  void* fn = anymdp_graph_step_fn(h, eff, mode, true);
  AnyMDPStepNode sn;
  return anymdp_pipe_graph_set(h, false, D, period, cycles, want, &h->pipe_key, [&](int g, int slot, int q, hipKernelNodeParams* np) {
    sn.fill(np, h, fn, h->d_ptick + q, g, slot, R, mode);
  }, fn != nullptr);
}

static __global__ __launch_bounds__(256) void anymdp_pipe_open_kernel(uint2* sr, int n, uint32_t tag, uint64_t* tick_words, int n_words,
                                                                      uint64_t tick_base, uint2* snap, uint32_t* snap_w, uint32_t* err,
                                                                      int bad_tag_env, int repairable) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    uint2 r = sr[i];
    r.x &= (1u << XV_ANYMDP_SR_TAG_SHIFT) - 1u;
    snap[i] = r;      // what the replay restores should a hand-off of this call expire (anymdp_replay_kernel)
    r.x |= (i == bad_tag_env ? ((tag + 77u) & 0x3FFFu) : tag) << XV_ANYMDP_SR_TAG_SHIFT;      // bad_tag_env: test hook, -1 otherwise
    sr[i] = r;
  }
  if (i < n_words) tick_words[i] = tick_base;
  // the error word as it is at entry; the HANDOFF bit leaves the word for the time of the call (a wave that finds it set takes
  // it for "this call has failed": xv_hand_aborted) and returns with the replay kernel
  if (i == 0 && repairable) { const uint32_t e = *err; snap_w[0] = e; snap_w[1] = 0u; snap_w[2] = 0u; *err = e & ~(uint32_t)XV_DEVERR_HANDOFF; }
}

// The whole ring cycles of a call, overlapped — MDP and token steps alike; *issued = steps issued (0: the caller takes the
// ordinary path for all of it).  What differs between the two comes from the caller:
//   fn                        the HAND kernel whose launches must fit on the device together
//   tokens                    which of the handle's two graph sets the lanes name (anymdp_pipe_lanes)
//   obs, n_obs                the call's observation ring and its element count (for the test hook anymdp_test_fail_kernel)
//   graphs(D, ring_cycles)    the call's graph set on D lanes, built or reused (anymdp_pipe_graphs / anymdp_tok_pipe_graphs)
//   replay(k, t0)             the family's replay kernel over the k steps issued from tick t0 -> launched
// Tags and tick words, then fork, launches and join (xv_pipe.h), then the replay kernel.
// -> XV_OK, or an error when a cycle went out in part (the streams are joined either way)
template <class Graphs, class Replay>
static int anymdp_pipe_call(xv_anymdp* h, int n_steps, int ring_period, int min_steps, const void* fn, bool tokens, int32_t* obs,
                            size_t n_obs, int* issued, Graphs&& graphs, Replay&& replay) {
  *issued = 0;
  // two or three launches resident at once, or the one-stream path (xv_pipe.h)
  int D = xv_pipe_preflight(n_steps, ring_period, min_steps, &h->backoff, &h->gate, fn, 256, (size_t)xv_div_up(h->a.n_env, 256),
                            h->eng->device, h->eng->stream);
  if (D == 0) return XV_OK;
  const int U = anymdp_pipe_setup(h, &D) ? graphs(D, n_steps / ring_period) : -1;
  if (U < 0) {
    (void)hipGetLastError();
    h->pipe_failed = true;
    return XV_OK;
  }
  if (U == 0) return XV_OK;      // too short for the graphs this handle holds: one stream
  const int cycles = n_steps / ring_period / U, period = ring_period * U;      // replays of the graph set, steps in each
  hipStream_t st = h->eng->stream;
  const int test_bad_tag = getenv("XV_PIPE_TEST_BAD_TAG") ? atoi(getenv("XV_PIPE_TEST_BAD_TAG")) : 0;   // tests: env 0's tag is wrong
  const int test_fail = getenv("XV_PIPE_TEST_FAIL") ? atoi(getenv("XV_PIPE_TEST_FAIL")) : 0;            // tests: see anymdp_test_fail_kernel
  h->fell_seen = __atomic_load_n(h->gate.h_issued + 1, __ATOMIC_ACQUIRE);
  const uint64_t t0 = h->eng->tick;
  // one launch opens the call: every record gets the tag of the first step (whatever ran since the last overlapped call
  // wrote the tag bits as 0), the graphs' tick words the base their head nodes advance by `period` first
  hipLaunchKernelGGL(anymdp_pipe_open_kernel, dim3(xv_div_up(h->a.n_env, 256)), dim3(256), 0, st, h->a.sr, h->a.n_env,
                     XV_ANYMDP_SR_TAG(t0), h->d_ptick, XV_PIPE_DEPTH_MAX, t0 - (uint64_t)period, h->d_snap, h->d_snap_w,
                     h->a.err, test_bad_tag ? 0 : -1, 1);
  const XvPipeLanes L = anymdp_pipe_lanes(h, tokens, h->gate.depth);
  h->ptick_valid = false;      // until the cycles have gone out
  if (hipGetLastError() != hipSuccess || !xv_pipe_fork(L)) {      // (nothing is joined here: see xv_pipe_fork)
    (void)hipGetLastError();
    h->pipe_failed = true;
    return XV_OK;
  }
  const XvPipeIssued r = xv_pipe_issue(L, &h->gate, cycles);
  const int k = r.cycles * period;
  h->eng->tick = t0 + (uint64_t)k;
  if (r.cycles < cycles) { (void)hipGetLastError(); h->pipe_failed = true; }
  *issued = k;
  if (r.broken || !r.joined) {
    (void)hipGetLastError();
    h->pipe_failed = true;
    xv_set_error("xv_anymdp_step_many: an overlapped ring cycle could be issued only in part; the envs' states are undefined");
    return XV_ERR_HIP;
  }
  if (k > 0) {
    // behind the join: should a hand-off of this call have expired, the call is replayed from its entry state on this
    // stream (anymdp_replay_kernel: a nearly empty launch otherwise) — an expiry costs time, never results
    if (test_fail)
      hipLaunchKernelGGL(anymdp_test_fail_kernel, dim3(xv_div_up(h->a.n_env, 256)), dim3(256), 0, st, h->a.sr, h->a.n_env, h->a.err, obs, n_obs);
    if (!replay(k, t0)) {
      (void)hipGetLastError();
      h->pipe_failed = true;      // (this call's hand-offs are flagged as before; the next calls take the one-stream path)
    }
    h->ptick_value = h->eng->tick; h->ptick_valid = true; h->graph_used_last = true; h->pipe_used_last = true;
  }
  return XV_OK;
}

static int anymdp_pipe_run(xv_anymdp* h, int n_steps, int period, const AnyMDPRings& R, int mode, int* issued) {
  static const int min_steps = getenv("XV_ANYMDP_PIPE_MIN_STEPS") ? atoi(getenv("XV_ANYMDP_PIPE_MIN_STEPS")) : XV_ANYMDP_PIPE_GRAPH_MIN;
  const int eff = anymdp_effective_search(h);
  return anymdp_pipe_call(h, n_steps, period, min_steps, anymdp_graph_step_fn(h, eff, mode, true), false, R.obs, (size_t)period * (size_t)h->a.n_env,
                          issued, [&](int D, int cycles) { return anymdp_pipe_graphs(h, D, period, cycles, R, mode); },
                          [&](int k, uint64_t t0) { return anymdp_launch_replay(h, eff, R.slot(0), period, k / period, mode, t0); });
}

// One handle per device may have the overlap on at a time, and never a view.  Two overlapped calls in flight at once can
// deadlock on the hardware queues: streams are mapped onto a few queues, each in order, and a launch that waits for a wave
// of a launch queued BEHIND another handle's waiting launch never gets it (measured: two views, each overlapped, 4.5 us
// per step instead of 3.6; four, their waits ran into the bound — scripts/devtools/probe_views_overlap.py).
// (the slot is the device's, shared with the other families' overlapped paths: engine.hip, xv_device_overlap_acquire)
extern "C" int xv_anymdp_set_step_many_overlap(xv_anymdp* h, int on) {
  XV_CHECK_ARG(h != nullptr && (on == 0 || on == 1));
  const int dev = h->eng->device;
  XV_CHECK_ARG(dev >= 0 && dev < 64);
  if (on) {
    if (h->parent != nullptr) {
      xv_set_error("xv_anymdp_set_step_many_overlap: not on a view (overlap the parent's step_many instead)");
      return XV_ERR_UNSUPPORTED;
    }
    if (!xv_device_overlap_acquire(dev, h)) {
      xv_set_error("xv_anymdp_set_step_many_overlap: another handle on device %d has the overlap on; one at a time", dev);
      return XV_ERR_UNSUPPORTED;
    }
    h->pipe_failed = false;
    xv_pipe_backoff_reset(&h->backoff, &h->gate);
    h->backoff_mixed.len = 0;      // (mixed.hip starts it over against its own replay counter)
  } else {
    xv_device_overlap_release(dev, h);
  }
  h->overlap = on;
  return XV_OK;
}

// 1: the last xv_anymdp_step_many overlapped its ring cycles, 0: it did not (off, odd period, per-lane search, device tick,
// graph mode 0), -1: the overlapped path failed on this handle and is no longer tried, -2: the last call overlapped, a
// hand-off expired and the call was replayed on one stream (results are right; meaningful once the stream has drained)
extern "C" int xv_anymdp_step_many_overlap_state(xv_anymdp* h) {
  if (!h) return 0;
  if (h->pipe_failed) return -1;
  if (h->overlap && h->pipe_used_last && h->gate.h_issued &&
      __atomic_load_n(h->gate.h_issued + 1, __ATOMIC_ACQUIRE) != h->fell_seen)
    return -2;
  return (h->overlap && h->pipe_used_last) ? 1 : 0;
}

extern "C" int xv_anymdp_step_many(xv_anymdp* h, int n_steps, int period, const int32_t* actions,
                                   int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                                   uint8_t* truncated, int32_t* final_obs, int autoreset_mode) {
  XV_CHECK_ARG(h && n_steps > 0 && period > 0);
  XV_CHECK_ARG(actions && obs && reward && reward_gt && terminated && truncated);
  XV_CHECK_ARG(autoreset_mode >= 0 && autoreset_mode <= 2);
  const AnyMDPRings R{(size_t)h->a.n_env, actions, obs, reward, reward_gt, terminated, truncated, final_obs};
  int k = 0;
  // whole ring cycles: replay the graph
  const int cycles = n_steps / period;
  h->pipe_used_last = false;
  if (h->overlap && h->graph_mode != 0 && !h->eng->dev_tick && !h->pipe_failed &&
      anymdp_effective_search(h) != XV_ANYMDP_SEARCH_BINARY) {
    XV_HIP(hipSetDevice(h->eng->device));
    h->graph_used_last = false;
    const int rc = anymdp_pipe_run(h, n_steps, period, R, autoreset_mode, &k);
    if (rc != XV_OK) return rc;
  }
  if (k == 0 && anymdp_many_prepare(h, n_steps, period, anymdp_graph_wanted(h, n_steps), true,
                                    [&] { return anymdp_ensure_graph(h, period, R, autoreset_mode); }))
    for (int c = 0; c < cycles && anymdp_many_cycle(h, h->graph_exec, period, true); ++c) k += period;
  for (; k < n_steps; ++k) {
    const int rc = anymdp_many_plain(h, k, period, R, autoreset_mode);
    if (rc != XV_OK) return rc;
  }
  return XV_OK;
}

// ONE graph for a ring cycle of all chains: K branches (the views' chains of `period` step nodes, all reading the parent's
// tick word) joined by the node that advances the word.  Kept on the parent.  R: the parent's rings.
static bool anymdp_ensure_chain_graph(xv_anymdp* p, xv_anymdp* const* views, int n_views, int period, const AnyMDPRings& R, int mode) {
  const int eff = anymdp_effective_search(p);
  decltype(p->cgraph_key) want;
  memset(&want, 0, sizeof want);
  want.period = period; want.mode = mode; want.search = eff; want.n_views = n_views;
  anymdp_ring_pointers(R, want.ptrs);
  want.bucket = (const void*)p->a.bucket;
  for (int v = 0; v < n_views; ++v) want.views[v] = (const void*)views[v];
  if (p->cgraph_exec && anymdp_key_same(want, p->cgraph_key)) return true;
  anymdp_drop_chain_graph(p);
  if (!p->d_tick && hipMalloc(&p->d_tick, sizeof(uint64_t)) != hipSuccess) return false;
  if (hipGraphCreate(&p->cgraph, 0) != hipSuccess) return false;
  hipGraphNode_t tails[XV_ANYMDP_MAX_CHAINS];
  for (int v = 0; v < n_views; ++v) {
    tails[v] = nullptr;
    if (!anymdp_add_chain(views[v], p->cgraph, &tails[v], p->d_tick, eff, period, R.shifted((size_t)views[v]->view_lo), mode)) return false;
  }
  if (!anymdp_add_tick_node(p->cgraph, tails, n_views, p->d_tick, period)) return false;
  if (hipGraphInstantiate(&p->cgraph_exec, p->cgraph, nullptr, nullptr, 0) != hipSuccess) { p->cgraph_exec = nullptr; return false; }
  anymdp_key_store(&p->cgraph_key, want);
  return true;
}

// xv_anymdp_step_many with the envs stepped as K independent chains: views[c] (xv_anymdp_view) covers a contiguous range
// of the parent's envs, the K ranges tile it in order.  Step k of chain c depends on step k - 1 of chain c only — so the
// chains run on their own streams (how = 0: each replays its own cycle graph, or plain launches when graphs are off) or as
// the K branches of one graph on the parent's stream (how = 1), and the launch-to-launch gap of one chain (an empty launch
// of this grid is 2.7 of the step's 5.0 us) is covered by the other chains' table lines in flight.  Same launch ticks and
// the same per-env Philox counters as one chain: every output, the env records and the parent's tick afterwards equal
// xv_anymdp_step_many's bit for bit.  Arrays are the parent's [period][parent n_env] rings.  Stream order: the chains start
// behind what the parent's stream holds at the call and the parent's stream waits for all of them before it goes on.
// Host tick only (device-tick engines: XV_ERR_UNSUPPORTED).
extern "C" int xv_anymdp_step_many_chains(xv_anymdp* p, xv_anymdp* const* views, int n_views, int how, int n_steps, int period,
                                          const int32_t* actions, int32_t* obs, float* reward, float* reward_gt,
                                          uint8_t* terminated, uint8_t* truncated, int32_t* final_obs, int autoreset_mode) {
  XV_CHECK_ARG(p && views && n_views >= 1 && n_views <= XV_ANYMDP_MAX_CHAINS && (how == 0 || how == 1));
  XV_CHECK_ARG(n_steps > 0 && period > 0);
  XV_CHECK_ARG(actions && obs && reward && reward_gt && terminated && truncated);
  XV_CHECK_ARG(autoreset_mode >= 0 && autoreset_mode <= 2);
  int covered = 0;
  bool dev_tick = p->eng->dev_tick;
  for (int v = 0; v < n_views; ++v) {
    XV_CHECK_ARG(views[v] != nullptr && views[v]->parent == p && views[v]->view_lo == covered);
    covered += views[v]->a.n_env;
    dev_tick = dev_tick || views[v]->eng->dev_tick;
  }
  XV_CHECK_ARG(covered == p->a.n_env);
  if (dev_tick) {
    xv_set_error("xv_anymdp_step_many_chains: needs the host tick on the parent's and the views' engines");
    return XV_ERR_UNSUPPORTED;
  }
  // the parent's rings; a view steps its columns of them: Rv(v)
  const AnyMDPRings R{(size_t)p->a.n_env, actions, obs, reward, reward_gt, terminated, truncated, final_obs};
  auto Rv = [&](int v) { return R.shifted((size_t)views[v]->view_lo); };
  XV_HIP(hipSetDevice(p->eng->device));
  const uint64_t t0 = p->eng->tick;
  const int cycles = n_steps / period;
  p->graph_used_last = false;
  for (int v = 0; v < n_views; ++v) {      // the views follow the parent: search setting and launch tick
    views[v]->search = p->search;
    views[v]->graph_mode = p->graph_mode;
    views[v]->eng->tick = t0;
  }
  int k = 0;
  if (how == 1) {
    // the parent replays its chain graph: its own tick word and tick per cycle, the views' ticks at the end (failures not kept)
    if (anymdp_many_prepare(p, n_steps, period, p->graph_mode != 0, false,
                            [&] { return anymdp_ensure_chain_graph(p, views, n_views, period, R, autoreset_mode); }))
      for (int c = 0; c < cycles && anymdp_many_cycle(p, p->cgraph_exec, period, false); ++c) k += period;
    for (; k < n_steps; ++k) {           // what is left of the call: the parent's own launches
      const int rc = anymdp_many_plain(p, k, period, R, autoreset_mode);
      if (rc != XV_OK) return rc;
    }
    for (int v = 0; v < n_views; ++v) views[v]->eng->tick = t0 + (uint64_t)n_steps;
    return XV_OK;
  }
  // how = 0: fork
  if (!p->chain_ev) XV_HIP(hipEventCreateWithFlags(&p->chain_ev, hipEventDisableTiming));
  XV_HIP(hipEventRecord(p->chain_ev, p->eng->stream));
  bool all_graph = true;
  for (int v = 0; v < n_views; ++v) {
    xv_anymdp* h = views[v];
    if (h->eng->stream != p->eng->stream) XV_HIP(hipStreamWaitEvent(h->eng->stream, p->chain_ev, 0));
    // (graphs whenever they are on, whatever the batch size: the host tick is certain here; every view is prepared)
    all_graph = anymdp_many_prepare(h, n_steps, period, h->graph_mode != 0, true,
                                    [&] { return anymdp_ensure_graph(h, period, Rv(v), autoreset_mode); }) && all_graph;
  }
  int rc = XV_OK;
  if (all_graph) {
    for (int c = 0; c < cycles && all_graph; ++c) {
      for (int v = 0; v < n_views; ++v) all_graph = anymdp_many_cycle(views[v], views[v]->graph_exec, period, true) && all_graph;
      if (all_graph) k += period;
    }
    p->graph_used_last = k > 0;
  }
  // a graph launch that failed mid-cycle leaves the chains at different steps: bring every chain to the furthest one
  for (int v = 0; v < n_views; ++v) k = (int)(views[v]->eng->tick - t0) > k ? (int)(views[v]->eng->tick - t0) : k;
  for (int v = 0; v < n_views && rc == XV_OK; ++v)
    for (int kk = (int)(views[v]->eng->tick - t0); kk < k && rc == XV_OK; ++kk)
      rc = anymdp_many_plain(views[v], kk, period, Rv(v), autoreset_mode);
  for (; k < n_steps && rc == XV_OK; ++k)
    for (int v = 0; v < n_views && rc == XV_OK; ++v) rc = anymdp_many_plain(views[v], k, period, Rv(v), autoreset_mode);
  // join (also after an error: the parent's stream must not run ahead of launches already issued)
  for (int v = 0; v < n_views; ++v) {
    xv_anymdp* h = views[v];
    if (h->eng->stream == p->eng->stream) continue;
    if (!h->chain_ev && hipEventCreateWithFlags(&h->chain_ev, hipEventDisableTiming) != hipSuccess) { rc = rc == XV_OK ? XV_ERR_HIP : rc; continue; }
    if (hipEventRecord(h->chain_ev, h->eng->stream) != hipSuccess ||
        hipStreamWaitEvent(p->eng->stream, h->chain_ev, 0) != hipSuccess)
      rc = rc == XV_OK ? XV_ERR_HIP : rc;
  }
  if (rc == XV_ERR_HIP) xv_set_error("xv_anymdp_step_many_chains: joining the chains failed: %s", hipGetErrorString(hipGetLastError()));
  if (rc == XV_OK) p->eng->tick = t0 + (uint64_t)n_steps;
  return rc;
}

// the graph set of the overlapped token step: HAND instantiations of the cooperative kernel
static int anymdp_tok_pipe_graphs(xv_anymdp* h, int D, int period, int cycles, const AnyMDPTokRings& R, int mode) {
  decltype(h->tpipe_key) want;
  memset(&want, 0, sizeof want);
  want.period = period; want.mode = mode; want.fmt = h->a.bfmt; want.d_obs = h->d_obs; want.d_act = h->d_act;
  anymdp_ring_pointers(R, want.ptrs);
  want.bucket = (const void*)h->a.bucket; want.obs_bucket = (const void*)h->obs_bucket;
  want.seed = h->eng->seed; want.gid_base = h->eng->env_id_base;
  void* fn = anymdp_tok_hand_fn(h);
  AnyMDPArgs a;
  AnyMDPTokArgs KA{h->obs_cdf, h->n_obs, h->d_obs, h->d_act, h->obs_bucket};
  AnyMDPTokIO io;
  int md = mode;
  void* params[] = {&a, &KA, &io, &md};
  return anymdp_pipe_graph_set(h, true, D, period, cycles, want, &h->tpipe_key, [&](int g, int slot, int q, hipKernelNodeParams* np) {
    a = h->a;
    a.seed = h->eng->seed; a.gid_base = h->eng->env_id_base;
    a.tick = (uint64_t)g; a.tick_dev = h->d_ptick + q;
    io = R.slot(h, slot);
    np->func = fn; np->gridDim = dim3(xv_div_up(h->a.n_env, 256)); np->blockDim = dim3(256); np->kernelParams = params;
  });
}

// n_steps token steps issued from C over ring buffers: step k reads actions slot k % period ([period][n_env][d_act]) and
// writes slot k % period of the outputs (obs / final_obs [period][n_env][d_obs], the others [period][n_env]); equals
// n_steps calls of xv_anymdp_step_tokens (a Python / ctypes loop costs more per call than the 10-20 us kernel).
// With xv_anymdp_set_step_many_overlap on, whole cycles of an even period (calls of >= 64 steps, cooperative kernel, host
// tick) are issued on two streams with the hand-off through the env records, as xv_anymdp_step_many's.
extern "C" int xv_anymdp_step_tokens_many(xv_anymdp* h, int n_steps, int period, const int32_t* action, int32_t* obs,
                                          float* reward, float* reward_gt, uint8_t* terminated, uint8_t* truncated,
                                          int32_t* final_obs, int autoreset_mode) {
  XV_CHECK_ARG(h && h->obs_cdf && n_steps > 0 && period > 0);
  XV_CHECK_ARG(action && obs && reward && reward_gt && terminated && truncated);
  XV_CHECK_ARG(autoreset_mode >= 0 && autoreset_mode <= 2);
  const AnyMDPTokRings R{action, obs, reward, reward_gt, terminated, truncated, final_obs};
  int k = 0;
  h->pipe_used_last = false;
  if (h->overlap && !h->eng->dev_tick && !h->pipe_failed && anymdp_tok_coop(h) && hipSetDevice(h->eng->device) == hipSuccess) {
    // (the minimum call length here is the constant: XV_ANYMDP_PIPE_MIN_STEPS moves it for the MDP steps only)
    const int rc = anymdp_pipe_call(h, n_steps, period, XV_ANYMDP_PIPE_GRAPH_MIN, anymdp_tok_hand_fn(h), true, R.obs,
                                    (size_t)period * (size_t)h->a.n_env * (size_t)h->d_obs, &k,
                                    [&](int D, int cycles) { return anymdp_tok_pipe_graphs(h, D, period, cycles, R, autoreset_mode); },
                                    [&](int kk, uint64_t t0) { return anymdp_tok_launch_replay(h, R.slot(h, 0), period, kk, autoreset_mode, t0); });
    if (rc != XV_OK) return rc;
  }
  for (; k < n_steps; ++k) {
    anymdp_bind_rng(h, 1);
    const int rc = anymdp_tok_launch_step<false>(h, R.slot(h, k % period), autoreset_mode);
    if (rc != XV_OK) return rc;
  }
  return XV_OK;
}
