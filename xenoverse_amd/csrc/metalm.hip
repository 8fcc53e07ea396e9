// metalm.hip — MetaLMV3 on the device: the reference's MetaLMV3Env (xenoverse/metalang/metalangv3.py:4-42) over its RandomLM
// (xenoverse/utils/random_nn.py:218-344) and the three decoders (:193-216).  Host restatement and the full statement of the
// semantics: xenoverse_amd/metalang/lm_host.py.  An ENV is one RandomLM task (emb [V][E] = layer_norm of the encoder's
// columns, W_h [H][H+E], b_h [H], W_d [V][H], b_d [V]) with a cached hidden state (what the last query left) and that query.
// Per token of a pass, in fp64:
//   :257-258  h = tanh(W_h concat(h, emb[tok]) + b_h)
//   :259-263  logits = W_d h + b_d + echo_bias;  logits[stop] += stop_bias;  logits[function tokens] = -1e6
//   :264-268  stop_bias: -1e6 at the first token, then 0.02, 0.04, ...;  echo_bias[tok] -= 0.05
//   softmax :193-198   e = exp((logits - max) / T);  greedy :208-216 the same at T = 1, and argmax unless the draw is 0;
//   rnd :200-206       logits[1:] below -1e5 become 0, e = exp(logits);  label :336-341  e = exp(logits), argmax, p[given]
//   the draw           p = e / sum(e); cdf = cumsum(p) / cumsum(p)[-1]; token = first v with cdf[v] > u (numpy's choice)
//   ppl               -log(max(p[token], 1e-10)), the stop step included; a pass reports the mean
//
// Kernel: ONE WAVE PER PASS, so a token step has no workgroup barrier.  reset and policy run one pass per env (a 64-thread
// workgroup); step runs four — the teacher-forced label pass, the greedy pass, the rnd pass and, unless `cached`, the next
// query — as the four waves of one workgroup, which meet once for the reward: they are independent, because the three
// answer passes start from the cached state and the query from zero.  Lane j owns hidden rows j and j + 64, then vocabulary
// columns j + 64 c (c < 4).  W_h and W_d come TRANSPOSED ([H+E][H], [H][V]) so that the lanes' loads of one k are adjacent.
// The hidden state lives in LDS (one row of H per wave: every lane reads all of it); the tables are copied to LDS at the
// start where they fit LM_TAB_CAP doubles (template TL), otherwise read through L2.  Sum and CDF by the DPP wave scan;
// ballot + first set bit for the first cut above u; argmax by a butterfly over (value, index).  Uniforms (or the given
// tokens) are fetched, and tokens written out, 64 positions at a time.  The recurrence is the host's bit for bit where
// H is a multiple of 4: the dot products run in the four FMA chains of the BLAS matvec behind numpy's `@` (k mod 4,
// summed (0 + 2) + (1 + 3), then its tail of (H + E) mod 4 terms), and tanh is lm_tanh below.  Past the hidden state nothing feeds back, and there the scan adds
// in tree order where numpy adds left to right, exp and log are the device's: DESIGN.md §3.7.  -ffp-contract=off: every
// FMA is written out.
//
// Free-running draws: u = xv_u53 of Philox words keyed by (engine seed, env_id_base + env, the call's tick, XV_DRAW_METALM,
// sub = pass kind << 16 | position >> 1): words 0,1 for an even position, 2,3 for an odd one.
#include "philox.h"
#include "xv_common.h"

#define XV_DRAW_METALM 9u

#define LM_V_MIN 12
#define LM_V_MAX 256
#define LM_H_MAX 128
#define LM_E_MAX 64
#define LM_LEN_MAX 1024
#define LM_NC (LM_V_MAX / 64)
#define LM_TAB_CAP 4096      // emb, W_h, b_h, W_d, b_d of the workgroup's task are copied to LDS up to this many doubles

enum { LM_QUERY = 0, LM_POLICY = 1, LM_LABEL = 2, LM_GREEDY = 3, LM_LOW = 4 };
enum { LM_MODE_RESET = 0, LM_MODE_POLICY = 1, LM_MODE_STEP = 2 };

struct LMArgs {
  const double* emb;      // [n_task][V][E]
  const double* w_h;      // [n_task][H+E][H]   W_h transposed
  const double* b_h;      // [n_task][H]
  const double* w_d;      // [n_task][H][V]     W_d transposed
  const double* b_d;      // [n_task][V]
  const int32_t* env_task;   // [N]
  uint64_t fmask[LM_NC];  // bit v & 63 of word v >> 6: v is a function token
  int n_task, N, V, E, H, max_len, stop, tab_n;
  int32_t* query;         // [N][max_len]  state: the current query
  int32_t* query_len;     // [N]
  double* cache;          // [N][H]        state: the hidden state the query left
  int32_t* steps;         // [N]
  uint64_t seed, gid_base, tick;
  const uint64_t* tick_dev;
  uint32_t* err;
};

struct LMCall {
  int mode;
  const double* u[4];        // per wave of the workgroup: [N][max_len + 1] injected uniforms or nullptr (Philox)
  const double* temp;        // policy: [N]
  const int32_t* ans;        // step: the action [N][max_len]
  const int32_t* ans_len;    // [N]
  const uint8_t* cached;     // step: [N] or nullptr (none)
  int32_t* out_tok[4];       // per wave: tokens out, row stride out_stride[w]; nullable
  int32_t* out_len[4];       // [N]; nullable
  int out_stride[4];
  double* ppl;               // step: [3][N] ppl, ppl_min, ppl_max; nullable
  double* reward;            // step: [N]
  int32_t* steps_out;        // step: [N]; nullable
};

// One DPP move of a double (two dwords); a lane the control leaves without a source, or a row the mask excludes, reads 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double lm_dpp(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xF, false);
  return __hiloint2double(hi, lo);
}

// inclusive scan over the wave's 64 lanes: four shifts inside the rows of 16, then the rows' totals carried over
__device__ __forceinline__ double lm_wave_scan(double x) {
  x += lm_dpp<0x111, 0xF>(x);      // row_shr:1
  x += lm_dpp<0x112, 0xF>(x);      // row_shr:2
  x += lm_dpp<0x114, 0xF>(x);      // row_shr:4
  x += lm_dpp<0x118, 0xF>(x);      // row_shr:8
  x += lm_dpp<0x142, 0xA>(x);      // row_bcast:15 -> rows 1 and 3
  x += lm_dpp<0x143, 0xC>(x);      // row_bcast:31 -> rows 2 and 3
  return x;
}

__device__ __forceinline__ double lm_lane(double x, int l) {      // lane l's x, to every lane (l is wave-uniform)
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

__device__ __forceinline__ double lm_wave_max(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m, 64));
  return x;
}

// what one wave's stores to its LDS row must pass before its other lanes read them
__device__ __forceinline__ void lm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tanh as NumPy's float64 loop computes it (the vectorised loop of its umath, one table and one polynomial per half octave
// of |x|, FMA throughout): row k of the table holds, for the 16 intervals [2^-3 .. 2^5) cut at 1 and 1.5 times a power of
// two (below 2^-3: interval 0, from 24 on: interval 15, where the result is 1), the expansion point b (k = 0) and the
// coefficient c(k-1) of  tanh|x| = c0 + y (c1 + y (c2 + ... y c16)),  y = |x| - b.  The recurrence is chaotic, so nothing
// short of the host's own roundings follows the host; with these the hidden state is the host's bit for bit.
static __device__ const unsigned long long lm_tanh_tab[18 * 16] = {
    0x0000000000000000ull, 0x3fcc000000000000ull, 0x3fd4000000000000ull, 0x3fdc000000000000ull,      // b
    0x3fe4000000000000ull, 0x3fec000000000000ull, 0x3ff4000000000000ull, 0x3ffc000000000000ull,
    0x4004000000000000ull, 0x400c000000000000ull, 0x4014000000000000ull, 0x401c000000000000ull,
    0x4024000000000000ull, 0x402c000000000000ull, 0x4034000000000000ull, 0x0000000000000000ull,
    0x0000000000000000ull, 0x3fcb8fd0416a7c92ull, 0x3fd35f98a0ea650eull, 0x3fda5729ee488037ull,      // c0
    0x3fe1bf47eabb8f95ull, 0x3fe686650b8c2015ull, 0x3feb2523bb6b2deeull, 0x3fee1fbf97e33527ull,
    0x3fef9258260a71c2ull, 0x3feff112c63a9077ull, 0x3fefff419668df11ull, 0x3feffffc832750f2ull,
    0x3feffffffdc96f35ull, 0x3fefffffffffcf58ull, 0x3ff0000000000000ull, 0x3ff0000000000000ull,
    0x3ff0000000000000ull, 0x3fee842ca3f08532ull, 0x3fed11574af58f1bull, 0x3fea945b9c24e4f9ull,      // c1
    0x3fe6284c3374f815ull, 0x3fe02500a09f8d6eull, 0x3fd1f25131e3a8c0ull, 0x3fbd22ca1c24a139ull,
    0x3f9b3afe1fba5c76ull, 0x3f6dd37d19b22b21ull, 0x3f27ccec13a9ef96ull, 0x3ecbe6c3f33250aeull,
    0x3e41b4865394f75full, 0x3d8853f01bda5f28ull, 0x3c73953c0197ef58ull, 0x0000000000000000ull,
    0xbbf0b3ea3fdfaa19ull, 0xbfca48aaeb53bc21ull, 0xbfd19921f4329916ull, 0xbfd5e0f09bef8011ull,      // c2
    0xbfd893b59c35c882ull, 0xbfd6ba7cb7576538ull, 0xbfce7291743d7555ull, 0xbfbb6d85a01efb80ull,
    0xbf9addae58c7141aull, 0xbf6dc59376c7aa19ull, 0xbf27cc5e74677410ull, 0xbecbe6c0e8b4cc87ull,
    0xbe41b486526b0565ull, 0xbd8853f01bef63a4ull, 0xbc73955be519be31ull, 0x0000000000000000ull,
    0xbfd5555555555555ull, 0xbfd183afc292ba11ull, 0xbfcc1a4b039c9bfaull, 0xbfc16e1e6d8d0be6ull,      // c3
    0xbf92426c751e48a2ull, 0x3fb4f152b2bad124ull, 0x3fbbba40cbef72beull, 0x3fb01ba038be6a3dull,
    0x3f916df44871efc8ull, 0x3f63c6869dfc8870ull, 0x3f1fb9aef915d828ull, 0x3ec299d1e27c6e11ull,
    0x3e379b5ddcca334cull, 0x3d8037f57bc62c9aull, 0x3c6a2d4b50a2cff7ull, 0x0000000000000000ull,
    0xbce6863ee44ed636ull, 0x3fc04dcd0476c75eull, 0x3fc43d3449a80f08ull, 0x3fc5c26f3699b7e7ull,      // c4
    0x3fc1a686f6ab2533ull, 0x3faf203c316ce730ull, 0xbf89c7a02788557cull, 0xbf98157e26e0d541ull,
    0xbf807b55c1c7d278ull, 0xbf53a18d5843190full, 0xbf0fb6bbc89b1a5bull, 0xbeb299c9c684a963ull,
    0xbe279b5dd4fb3d01ull, 0xbd7037f57ae72aa6ull, 0xbc5a2ca2bba78e86ull, 0x0000000000000000ull,
    0x3fc1111111112ab5ull, 0x3fb5c19efdfc08adull, 0x3fa74c98dc34fbacull, 0xbf790d6a8eff0a77ull,      // c5
    0xbfac3c021789a786ull, 0xbfae2196b7326859ull, 0xbf93a7a011ff8c2aull, 0x3f6e4709c7e8430eull,
    0x3f67682afa611151ull, 0x3f3ef2ee77717cbfull, 0x3ef95a4482f180b7ull, 0x3e9dc2c27da3b603ull,
    0x3e12e2afd9f7433eull, 0x3d59f320348679baull, 0x3c44b61d9bbcc940ull, 0x0000000000000000ull,
    0xbda1ea19ddddb3b4ull, 0xbfb0b8df995ce4dfull, 0xbfb2955cf41e8164ull, 0xbfaf9d05c309f7c6ull,      // c6
    0xbf987d27ccff4291ull, 0x3f8b2ca62572b098ull, 0x3f8f1cf6c7f5b00aull, 0x3f60379811e43dd5ull,
    0xbf4793826f78537eull, 0xbf2405695e36240full, 0xbee0e08de39ce756ull, 0xbe83d709ba5f714eull,
    0xbdf92e3fc5ee63e0ull, 0xbd414cc030f2110eull, 0xbc2ba022e8d82a87ull, 0x0000000000000000ull,
    0xbfaba1ba1990520bull, 0xbf96e37bba52f6fcull, 0x3ecff7df18455399ull, 0x3f97362834d33a4eull,      // c7
    0x3f9e7f8380184b45ull, 0x3f869543e7c420d4ull, 0xbf7326bd4914222aull, 0xbf5fc15b0a9d98faull,
    0x3f14cffcfa69fbb6ull, 0x3f057e48e5b79d10ull, 0x3ec33b66d7d77264ull, 0x3e66ac4e578b9b10ull,
    0x3ddcc74b8d3d5c42ull, 0x3d23c589137f92b4ull, 0x3c107f8e2c8707a1ull, 0x0000000000000000ull,
    0xbe351ca7f096011full, 0x3f9eaaf3320c3851ull, 0x3f9cf823fe761fc1ull, 0x3f9022271754ff1full,      // c8
    0xbf731fe77c9c60afull, 0xbf84a6046865ec7dull, 0xbf4ca3f1f2b9192bull, 0x3f4c77dee0afd227ull,
    0x3f04055bce68597aull, 0xbee2bf0cb4a71647ull, 0xbea31eaafe73efd5ull, 0xbe46abb02c4368edull,
    0xbdbcc749ca8079ddull, 0xbd03c5883836b9d2ull, 0xbbf07a5416264aecull, 0x0000000000000000ull,
    0x3f9664f94e6ac14eull, 0xbf94d3343bae39ddull, 0xbf7bc748e60df843ull, 0xbf8c89372b43ba85ull,      // c9
    0xbf8129a092de747aull, 0x3f60c85b4d538746ull, 0x3f5be9392199ec18ull, 0xbf2a0c68a4489f10ull,
    0xbf00462601dc2faaull, 0x3eb7b6a219dea9f4ull, 0x3e80cbcc8d4c5c8aull, 0x3e2425bb231a5e29ull,
    0x3d9992a4beac8662ull, 0x3ce191ba5ed3fb67ull, 0x3bc892450bad44c4ull, 0x0000000000000000ull,
    0xbea8c4c1fd7852feull, 0xbfccce16b1046f13ull, 0xbf81a16f224bb7b6ull, 0xbf62cbf00406bc09ull,      // c10
    0x3f75b29bb02cf69bull, 0x3f607df0f9f90c17ull, 0xbf4b852a6e0758d5ull, 0xbf0078c63d1b8445ull,
    0x3eec12eadd55be7aull, 0xbe6fa600f593181bull, 0xbe5a3c935dce3f7dull, 0xbe001c6d95e3ae96ull,
    0xbd74755a00ea1fd3ull, 0xbcbc1c6c063bb7acull, 0xbba3be9a4460fe00ull, 0x0000000000000000ull,
    0xbf822404577aa9ddull, 0x403d8b07f7a82aa3ull, 0xbf9f44ab92fbab0aull, 0x3fb2eac604473d6aull,      // c11
    0x3f45f87d903aaac8ull, 0xbf5e104671036300ull, 0x3f19bc98ddf0f340ull, 0x3f0d4304bc9246e8ull,
    0xbed13c415f7b9d41ull, 0xbe722b8d9720cdb0ull, 0x3e322666d739bec0ull, 0x3dd76a553d7e7918ull,
    0x3d4de0fa59416a39ull, 0x3c948716cf3681b4ull, 0x3b873f9f2d2fda99ull, 0x0000000000000000ull,
    0xbefdd99a221ed573ull, 0x4070593a3735bab4ull, 0xbfccab654e44835eull, 0x3fd13ed80037dbacull,      // c12
    0xbf6045b9076cc487ull, 0x3f2085ee7e8ac170ull, 0x3f23524622610430ull, 0xbeff12a6626911b4ull,
    0x3eab9008bca408afull, 0x3e634df71865f620ull, 0xbe05bb1bcf83ca73ull, 0xbdaf2ac143fb6762ull,
    0xbd23eae52a3dbf57ull, 0xbc6b5e3e9ca0955eull, 0xbb5eca68e2c1ba2eull, 0x0000000000000000ull,
    0x3f6e3be689423841ull, 0xc0d263511f5baac1ull, 0x40169f73b15ebe5cull, 0xc025c1dd41cd6cb5ull,      // c13
    0xbf58fd89fe05e0d1ull, 0x3f73f7af01d5af7aull, 0xbf1e40bdead17e6bull, 0x3ee224cd6c4513e5ull,
    0xbe24b645e68eeaa3ull, 0xbe4abfebfb72bc83ull, 0x3dd51c38f8695ed3ull, 0x3d8313ac38c6832bull,
    0x3cf7787935626685ull, 0x3c401ffc49c6bc29ull, 0xbabf0b21acfa52abull, 0x0000000000000000ull,
    0xbf2a1306713a4f3aull, 0xc1045e509116b066ull, 0x4041fab9250984ceull, 0xc0458d090ec3de95ull,      // c14
    0xbf74949d60113d63ull, 0x3f7c9fd6200d0adeull, 0x3f02cd40e0ad0a9full, 0xbe858ab8e019f311ull,
    0xbe792fa6323b7cf8ull, 0x3e2df04d67876402ull, 0xbd95c72be95e4d2cull, 0xbd55a89c30203106ull,
    0xbccad6b3bb9eff65ull, 0xbc12705ccd3dd884ull, 0xba8e0a4c47ae75f5ull, 0x0000000000000000ull,
    0xbf55d7e76dc56871ull, 0x41528c38809c90c7ull, 0xc076d57fb5190b02ull, 0x4085f09f888f8adaull,      // c15
    0x3fa246332a2fcba5ull, 0xbfb29d851a896fcdull, 0x3ed9065ae369b212ull, 0xbeb8e1ba4c98a030ull,
    0x3e6ffd0766ad4016ull, 0xbe0c63c29f505f5bull, 0xbd7fab216b9e0e49ull, 0x3d2826b62056aa27ull,
    0x3ca313e31762f523ull, 0x3bea37aa21895319ull, 0x3ae5c7f1fd871496ull, 0x0000000000000000ull,
    0x3f35e67ab76a26e7ull, 0x41848ee0627d8206ull, 0xc0a216d618b489ecull, 0x40a5b89107c8af4full,      // c16
    0x3fb69d8374520edaull, 0xbfbded519f981716ull, 0xbef02d288b5b3371ull, 0x3eb290981209c1a6ull,
    0xbe567e924bf5ff6eull, 0x3de3f7f7de6b0eb6ull, 0x3d69ed18bae3ebbcull, 0xbcf7534c4f3dfa71ull,
    0xbc730b73f1eaff20ull, 0xbbba2cff8135d462ull, 0xbab5a71b5f7d9035ull, 0x0000000000000000ull,
};

__device__ __forceinline__ double lm_tanh(double x, const double* tt) {      // tt: the table, in LDS
  const long long bits = __double_as_longlong(x);
  long long i = (bits & 0x7ff8000000000000ll) - 0x3fc0000000000000ll;
  i = i < 0 ? 0 : i > 0x0078000000000000ll ? 0x0078000000000000ll : i;
  const double* c = tt + (int)(i >> 51);
  const double y = fabs(x) - c[0];
  double r = fma(c[17 * 16], y, c[16 * 16]);
#pragma unroll
  for (int k = 15; k >= 1; --k) r = fma(r, y, c[k * 16]);
  return __longlong_as_double(__double_as_longlong(r) | (bits & (long long)0x8000000000000000ull));
}

#include "metalm_pass.h"

template <bool TL>
__global__ __launch_bounds__(256) void metalm_kernel(LMArgs P, LMCall C) {
  extern __shared__ double lm_tab[];
  __shared__ double lm_hs[4][LM_H_MAX];
  __shared__ double lm_mean[4];
  __shared__ double lm_tt[18 * 16];
  for (int i = threadIdx.x; i < 18 * 16; i += blockDim.x) lm_tt[i] = __longlong_as_double((long long)lm_tanh_tab[i]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int env = blockIdx.x;
  const int H = P.H, max_len = P.max_len;
  const int kind = C.mode == LM_MODE_STEP ? (wave == 0 ? LM_LABEL : wave == 1 ? LM_GREEDY : wave == 2 ? LM_LOW : LM_QUERY)
                                          : (C.mode == LM_MODE_RESET ? LM_QUERY : LM_POLICY);
  uint32_t err = 0u;
  const double *emb, *w_h, *b_h, *w_d, *b_d;
  lm_tables<TL>(P, env, lm_tab, err, emb, w_h, b_h, w_d, b_d);
  double* hs = lm_hs[wave];
  // every pass but the query starts from the cached state; the query wave overwrites that state only at its end, behind
  // this barrier
  for (int j = lane; j < H; j += 64) hs[j] = kind == LM_QUERY ? 0.0 : P.cache[(size_t)env * H + j];
  __syncthreads();

  const bool skip = kind == LM_QUERY && C.mode == LM_MODE_STEP && C.cached != nullptr && C.cached[env] != 0;
  int n_ans = 0;
  if (kind == LM_LABEL) {
    n_ans = C.ans_len[env];
    if (n_ans < 0 || n_ans > max_len) { err |= XV_DEVERR_ACTION_RANGE; n_ans = n_ans < 0 ? 0 : max_len; }
  }
  const double* u_in = C.u[wave];
  int32_t* out = C.out_tok[wave];
  const int stride = C.out_stride[wave];
  const uint64_t tick = xv_launch_tick(P.tick, P.tick_dev);
  const uint64_t gid = P.gid_base + (uint64_t)env;
  const double temp0 = kind == LM_QUERY ? 10.0 : kind == LM_POLICY ? C.temp[env] : 1.0;
  const double temp1 = kind == LM_POLICY ? temp0 : 1.0;
  if (kind == LM_POLICY && !(temp0 > 0.0 && temp0 <= 1.0e300)) err |= XV_DEVERR_NONFINITE;

  LMPass A;
  A.kind = kind; A.skip = skip; A.n_ans = n_ans;
  A.ans = C.ans ? C.ans + (size_t)env * max_len : nullptr;
  A.u = u_in ? u_in + (size_t)env * (max_len + 1) : nullptr;
  A.gid = gid; A.tick = tick; A.temp0 = temp0; A.temp1 = temp1;
  A.dst = kind == LM_QUERY ? P.query + (size_t)env * max_len : out ? out + (size_t)env * stride : nullptr;
  A.dst2 = nullptr; A.at = A.at2 = A.cap = 0; A.fuse = false;
  lm_pass<false>(P, emb, w_h, b_h, w_d, b_d, hs, lm_tt, lane, A, err);
  const int n_step = A.n_step;
  const double ppl_sum = A.ppl_sum;
  int n_out = A.n_out;

  if (kind == LM_QUERY) {
    int32_t* q = P.query + (size_t)env * max_len;
    if (!skip) {
      for (int i = n_out + lane; i < max_len; i += 64) q[i] = 0;
      for (int j = lane; j < H; j += 64) P.cache[(size_t)env * H + j] = hs[j];
      if (lane == 0) P.query_len[env] = n_out;
    } else {
      n_out = P.query_len[env];
    }
    if (out) {      // the caller's copy of the state's query (the wave's own stores are visible to it in program order)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      for (int i = lane; i < stride; i += 64) out[(size_t)env * stride + i] = i < n_out ? q[i] : 0;
    }
  } else if (out) {
    for (int i = n_out + lane; i < stride; i += 64) out[(size_t)env * stride + i] = 0;
  }
  if (lane == 0 && C.out_len[wave]) C.out_len[wave][env] = n_out;

  if (C.mode == LM_MODE_STEP) {
    if (lane == 0) lm_mean[wave] = n_step ? ppl_sum / (double)n_step : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double ppl = lm_mean[0], ppl_min = lm_mean[1], ppl_max = lm_mean[2];
      C.reward[env] = (ppl_max - ppl_min) / fmax(ppl - ppl_min + 0.1, 1.0e-3) - 2.0;      // metalangv3.py:32
      if (C.ppl) {
        C.ppl[env] = ppl;
        C.ppl[(size_t)P.N + env] = ppl_min;
        C.ppl[2 * (size_t)P.N + env] = ppl_max;
      }
      const int st = P.steps[env] + 1;
      P.steps[env] = st;
      if (C.steps_out) C.steps_out[env] = st;
    }
  } else if (C.mode == LM_MODE_RESET && lane == 0) {
    P.steps[env] = 0;
  }
  if (err) atomicOr(P.err, err);
}

// ---- the training streams (xenoverse/metalang/generator_v3.py:48-173; host restatement: metalang/stream_host.py) ----------
// ONE WORKGROUP PER ENV runs round after round from the handle's state until its own data cursor reaches L (or max_rounds):
// no launch boundary, so no env waits for the batch's longest pass.  A sub-step is what policy() + step() do: wave 0 runs
// the policy pass with the label pass over its own answer fused into the token step (lm_pass), waves 1 and 2 the greedy and
// rnd passes, wave 3 the next query unless the sub-step is cached (QARA's first); they meet at ONE barrier, behind which
// every thread forms the reward from the four means.  What a sub-step leaves for that barrier (means, lengths, the query's
// hidden state) is kept twice, by the parity of the sub-step, so a wave that runs ahead never overwrites what a slower
// one has yet to read.  Tokens go straight to their place in the stream: the position of every piece of a round is known
// once the lengths before it are (the query's before the round, answer 1's before QARA's second sub-step).  Tokens at or
// past L are not stored.  Sub-step k draws its policy pass (and its temperature: pass kind 5, position 0) at tick + 2 k
// and the other passes at tick + 2 k + 1: the ticks the same policy() / step() calls would bind.
enum { LM_QA = XV_METALM_QA, LM_QAR = XV_METALM_QAR, LM_QARA = XV_METALM_QARA, LM_TEMP = 5 };
enum { LM_S = 0, LM_Q = 1, LM_A = 2, LM_R1 = 3, LM_RGT = 8, LM_REQ = 9, LM_RLT = 10 };

struct LMStream {
  int datatype, L, max_rounds, K, n_choice;
  const double* t_choices;   // [n_choice]
  const int32_t* t_index;    // [N][K] or nullptr (drawn)
  const double* u[4];        // policy, greedy, low, query: [N][K][max_len + 1] or nullptr (Philox)
  int32_t marks[11];         // s q a r1..r5 r> r= r<
  int32_t* data;             // [N][L]
  int32_t* label;            // [N][L]
  int32_t* filled;           // [N]
  int32_t* rounds;           // [N]
  double* reward;            // [N][K]; nullable
  int32_t* t_index_out;      // [N][K]; nullable
};

template <bool TL>
__global__ __launch_bounds__(256) void metalm_stream_kernel(LMArgs P, LMStream S) {
  extern __shared__ double lm_tab[];
  __shared__ double lm_hs[4][LM_H_MAX];
  __shared__ double lm_cache[2][LM_H_MAX];
  __shared__ double lm_mean[2][4];
  __shared__ int lm_len[2][4];
  __shared__ double lm_tt[18 * 16];
  for (int i = threadIdx.x; i < 18 * 16; i += blockDim.x) lm_tt[i] = __longlong_as_double((long long)lm_tanh_tab[i]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int env = blockIdx.x;
  const int H = P.H, max_len = P.max_len, L = S.L, K = S.K;
  const int kind = wave == 0 ? LM_POLICY : wave == 1 ? LM_GREEDY : wave == 2 ? LM_LOW : LM_QUERY;
  uint32_t err = 0u;
  const double *emb, *w_h, *b_h, *w_d, *b_d;
  lm_tables<TL>(P, env, lm_tab, err, emb, w_h, b_h, w_d, b_d);
  for (int j = threadIdx.x; j < H; j += blockDim.x) lm_cache[0][j] = P.cache[(size_t)env * H + j];
  __syncthreads();

  double* hs = lm_hs[wave];
  int32_t* data = S.data + (size_t)env * L;
  int32_t* label = S.label + (size_t)env * L;
  int32_t* query = P.query + (size_t)env * max_len;
  const uint64_t tick0 = xv_launch_tick(P.tick, P.tick_dev);
  const uint64_t gid = P.gid_base + (uint64_t)env;
  const int per = S.datatype == LM_QARA ? 2 : 1;
  const bool rewarded = S.datatype != LM_QA;
  int nq = P.query_len[env];
  if (nq < 0 || nq > max_len) { err |= XV_DEVERR_ACTION_RANGE; nq = nq < 0 ? 0 : max_len; }
  int cur = 0, d0 = 0, l0 = 0, k = 0, round = 0;
  int ad1 = 0, al1 = 0, n1 = 0;      // QARA: where answer 1 and its label went, and its length
  double r1 = 0.0;
  while (d0 < L && round < S.max_rounds) {
    for (int sub = 0; sub < per; ++sub, ++k) {
      const bool cached = per == 2 && sub == 0;
      const int par = k & 1;
      // data: q obs s a ACT ...;  label: obs s a LABEL ...;  QARA's second answer follows  s r a  behind the first
      const int ad = sub == 0 ? d0 + nq + 3 : ad1 + n1 + 3;
      const int al = sub == 0 ? l0 + nq + 2 : al1 + n1 + 4;
      int ti = -1;
      double temp = 1.0e-3;      // QA
      if (rewarded && kind == LM_POLICY) {      // the policy wave alone needs it (and its first thread reports it)
        if (S.t_index) {
          ti = S.t_index[(size_t)env * K + k];
          if ((unsigned)ti >= (unsigned)S.n_choice) { err |= XV_DEVERR_ACTION_RANGE; ti = 0; }
        } else {
          const xv_u32x4 w = xv_env_draw_sub(P.seed, gid, tick0 + 2 * (uint64_t)k, XV_DRAW_METALM, (uint32_t)LM_TEMP << 16);
          ti = (int)(xv_u53(w.x, w.y) * (double)S.n_choice);
          ti = ti < S.n_choice - 1 ? ti : S.n_choice - 1;
        }
        temp = S.t_choices[ti];
      }
      if (kind == LM_POLICY && !(temp > 0.0 && temp <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
      if (threadIdx.x == 0 && rewarded && S.t_index_out) S.t_index_out[(size_t)env * K + k] = ti;

      for (int j = lane; j < H; j += 64) hs[j] = kind == LM_QUERY ? 0.0 : lm_cache[cur][j];
      lm_wave_sync();
      if (kind == LM_QUERY && sub == 0) {      // the head of the round, by the wave that will overwrite the query
        for (int i = lane; i < nq; i += 64) {
          const int t = query[i];
          if (d0 + 1 + i < L) data[d0 + 1 + i] = t;
          if (l0 + i < L) label[l0 + i] = t;
        }
        if (lane == 0) {
          if (d0 < L) data[d0] = S.marks[LM_Q];
          if (d0 + nq + 1 < L) data[d0 + nq + 1] = S.marks[LM_S];
          if (d0 + nq + 2 < L) data[d0 + nq + 2] = S.marks[LM_A];
          if (l0 + nq < L) label[l0 + nq] = S.marks[LM_S];
          if (l0 + nq + 1 < L) label[l0 + nq + 1] = S.marks[LM_A];
        }
      }
      LMPass A;
      A.kind = kind;
      A.skip = kind == LM_QUERY ? cached : kind != LM_POLICY && !rewarded;
      A.n_ans = 0; A.ans = nullptr;
      const double* u_in = S.u[wave];
      A.u = u_in ? u_in + ((size_t)env * K + k) * (max_len + 1) : nullptr;
      A.gid = gid;
      A.tick = tick0 + 2 * (uint64_t)k + (kind == LM_POLICY ? 0 : 1);
      A.temp0 = kind == LM_QUERY ? 10.0 : kind == LM_POLICY ? temp : 1.0;
      A.temp1 = kind == LM_POLICY ? temp : 1.0;
      A.dst = kind == LM_POLICY ? data : kind == LM_QUERY ? query : nullptr;
      A.at = kind == LM_POLICY ? ad : 0;
      A.dst2 = kind == LM_POLICY ? label : nullptr;
      A.at2 = al;
      A.cap = kind == LM_POLICY ? L : max_len;
      A.fuse = rewarded && kind == LM_POLICY;
      lm_pass<true>(P, emb, w_h, b_h, w_d, b_d, hs, lm_tt, lane, A, err);
      if (kind == LM_QUERY && !cached) {
        for (int i = A.n_out + lane; i < max_len; i += 64) query[i] = 0;
        for (int j = lane; j < H; j += 64) lm_cache[cur ^ 1][j] = hs[j];
      }
      if (lane == 0) {
        const double sum = kind == LM_POLICY ? A.ppl_sum2 : A.ppl_sum;      // wave 0 reports the label pass
        lm_mean[par][wave] = A.n_step ? sum / (double)A.n_step : 0.0;
        lm_len[par][wave] = A.n_out;
      }
      __syncthreads();
      const int na = lm_len[par][0];
      double r = 0.0;
      if (rewarded) {
        const double ppl = lm_mean[par][0], ppl_min = lm_mean[par][1], ppl_max = lm_mean[par][2];
        r = (ppl_max - ppl_min) / fmax(ppl - ppl_min + 0.1, 1.0e-3) - 2.0;      // metalangv3.py:32
        if (threadIdx.x == 0 && S.reward) S.reward[(size_t)env * K + k] = r;
      }
      if (cached) {      // QARA's first sub-step: the reward token waits for the second
        ad1 = ad; al1 = al; n1 = na; r1 = r;
        continue;
      }
      int dn, ln;      // the cursors behind this round
      if (S.datatype == LM_QARA) {
        const double deta = r1 - r;      // generator_v3.py:97-104, in its order
        const int rt = deta > 0.20 ? S.marks[LM_RGT] : deta < 0.5 ? S.marks[LM_RLT] : S.marks[LM_REQ];
        dn = ad + na + 1;
        ln = al + na + 3;
        if (threadIdx.x == 0) {
          if (ad1 + n1 < L) data[ad1 + n1] = S.marks[LM_S];
          if (ad1 + n1 + 1 < L) data[ad1 + n1 + 1] = rt;
          if (ad1 + n1 + 2 < L) data[ad1 + n1 + 2] = S.marks[LM_A];
          if (ad + na < L) data[ad + na] = S.marks[LM_S];
          if (al1 + n1 + 1 < L) label[al1 + n1 + 1] = S.marks[LM_S];
          if (al1 + n1 + 2 < L) label[al1 + n1 + 2] = rt;
          if (al1 + n1 + 3 < L) label[al1 + n1 + 3] = S.marks[LM_A];
          if (al + na + 1 < L) label[al + na + 1] = S.marks[LM_S];
          if (al + na + 2 < L) label[al + na + 2] = S.marks[LM_Q];
        }
      } else if (S.datatype == LM_QAR) {
        const int rt = S.marks[LM_R1 + (r < 0.0 ? 0 : r < 0.5 ? 1 : r < 1.0 ? 2 : r < 2.0 ? 3 : 4)];      // :52-62
        dn = ad + na + 2;
        ln = al + na + 4;
        if (threadIdx.x == 0) {
          if (ad + na < L) data[ad + na] = S.marks[LM_S];
          if (ad + na + 1 < L) data[ad + na + 1] = rt;
          if (al + na + 1 < L) label[al + na + 1] = S.marks[LM_S];
          if (al + na + 2 < L) label[al + na + 2] = rt;
          if (al + na + 3 < L) label[al + na + 3] = S.marks[LM_Q];
        }
      } else {
        dn = ad + na + 1;
        ln = al + na + 2;
        if (threadIdx.x == 0) {
          if (ad + na < L) data[ad + na] = S.marks[LM_S];
          if (al + na < L) label[al + na] = S.marks[LM_S];
          if (al + na + 1 < L) label[al + na + 1] = S.marks[LM_Q];
        }
      }
      d0 = dn;
      l0 = ln < L ? ln : L;      // the label stream runs ahead of the data stream: keep its cursor in range
      nq = lm_len[par][3];
      cur ^= 1;
    }
    ++round;
  }
  // what max_rounds left unfilled is 0; the state the last sub-step left goes back to the handle
  const int df = d0 < L ? d0 : L;
  for (int i = df + (int)threadIdx.x; i < L; i += blockDim.x) data[i] = 0;
  for (int i = l0 + (int)threadIdx.x; i < L; i += blockDim.x) label[i] = 0;
  for (int j = threadIdx.x; j < H; j += blockDim.x) P.cache[(size_t)env * H + j] = lm_cache[cur][j];
  if (threadIdx.x == 0) {
    P.query_len[env] = nq;
    P.steps[env] += k;
    S.filled[env] = df;
    S.rounds[env] = round;
  }
  if (err) atomicOr(P.err, err);
}

#ifndef XV_KERNELS_ONLY
#include <new>

struct xv_metalm {
  xv_engine* eng;
  LMArgs a;
  bool task_set;
};

extern "C" int xv_metalm_create(xv_engine* e, int n_env, int n_vocab, int n_emb, int n_hidden, int max_len, int stop_token,
                                const int32_t* function_tokens, int n_function, xv_metalm** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(e != nullptr && n_env >= 1 && n_function >= 0 && (n_function == 0 || function_tokens != nullptr));
  const struct { const char* name; int v, lo, hi; } lim[4] = {{"n_vocab", n_vocab, LM_V_MIN, LM_V_MAX},
                                                              {"n_hidden", n_hidden, 1, LM_H_MAX},
                                                              {"n_emb", n_emb, 1, LM_E_MAX},
                                                              {"max_len", max_len, 1, LM_LEN_MAX}};
  for (int i = 0; i < 4; ++i)
    if (lim[i].v < lim[i].lo || lim[i].v > lim[i].hi) {
      xv_set_error("xv_metalm_create: %s = %d is outside the supported range %d .. %d", lim[i].name, lim[i].v, lim[i].lo,
                   lim[i].hi);
      return XV_ERR_UNSUPPORTED;
    }
  XV_CHECK_ARG(stop_token >= 0 && stop_token < n_vocab);
  xv_metalm* h = new (std::nothrow) xv_metalm();
  if (!h) {
    xv_set_error("xv_metalm_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  h->eng = e;
  h->task_set = false;
  LMArgs& a = h->a;
  a = LMArgs();
  a.N = n_env; a.V = n_vocab; a.E = n_emb; a.H = n_hidden; a.max_len = max_len; a.stop = stop_token;
  for (int i = 0; i < n_function; ++i) {
    const int t = function_tokens[i];
    if (t < 0 || t >= n_vocab) {
      delete h;
      xv_set_error("xv_metalm_create: function token %d is outside the vocabulary of %d", t, n_vocab);
      return XV_ERR_INVALID;
    }
    a.fmask[t >> 6] |= 1ull << (t & 63);
  }
  const int tab = n_vocab * n_emb + (n_hidden + n_emb) * n_hidden + n_hidden + n_hidden * n_vocab + n_vocab;
  a.tab_n = tab <= LM_TAB_CAP ? tab : 0;
  a.err = e->d_err;
  XV_HIP(hipSetDevice(e->device));
  const size_t nq = sizeof(int32_t) * (size_t)n_env * max_len, nc = sizeof(double) * (size_t)n_env * n_hidden,
               ni = sizeof(int32_t) * (size_t)n_env;
  hipError_t r = hipMalloc(&a.query, nq);
  if (r == hipSuccess) r = hipMalloc(&a.cache, nc);
  if (r == hipSuccess) r = hipMalloc(&a.query_len, ni);
  if (r == hipSuccess) r = hipMalloc(&a.steps, ni);
  if (r == hipSuccess) r = hipMemsetAsync(a.query, 0, nq, e->stream);
  if (r == hipSuccess) r = hipMemsetAsync(a.cache, 0, nc, e->stream);
  if (r == hipSuccess) r = hipMemsetAsync(a.query_len, 0, ni, e->stream);
  if (r == hipSuccess) r = hipMemsetAsync(a.steps, 0, ni, e->stream);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    xv_set_error("xv_metalm_create: the state of %d envs does not fit: %s", n_env, hipGetErrorString(r));
    if (a.query) (void)hipFree(a.query);
    if (a.cache) (void)hipFree(a.cache);
    if (a.query_len) (void)hipFree(a.query_len);
    if (a.steps) (void)hipFree(a.steps);
    delete h;
    return r == hipErrorOutOfMemory ? XV_ERR_NOMEM : XV_ERR_HIP;
  }
  *out = h;
  return XV_OK;
}

extern "C" int xv_metalm_destroy(xv_metalm* h) {
  if (!h) return XV_OK;
  (void)hipSetDevice(h->eng->device);
  (void)hipStreamSynchronize(h->eng->stream);
  (void)hipFree(h->a.query);
  (void)hipFree(h->a.cache);
  (void)hipFree(h->a.query_len);
  (void)hipFree(h->a.steps);
  delete h;
  return XV_OK;
}

extern "C" int xv_metalm_set_task(xv_metalm* h, int n_task, const double* emb, const double* w_h_t, const double* b_h,
                                  const double* w_d_t, const double* b_d, const int32_t* env_task) {
  XV_CHECK_ARG(h != nullptr && n_task >= 1);
  XV_CHECK_ARG(emb && w_h_t && b_h && w_d_t && b_d && env_task);
  LMArgs& a = h->a;
  a.n_task = n_task;
  a.emb = emb; a.w_h = w_h_t; a.b_h = b_h; a.w_d = w_d_t; a.b_d = b_d; a.env_task = env_task;
  h->task_set = true;
  return XV_OK;
}

static int lm_launch(xv_metalm* h, const char* who, LMCall& c) {
  if (!h->task_set) {
    xv_set_error("%s: no task set (xv_metalm_set_task)", who);
    return XV_ERR_INVALID;
  }
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  LMArgs a = h->a;
  const XvTickBind tb = xv_engine_bind_tick(e, 1);
  a.tick = tb.tick;
  a.tick_dev = tb.tick_dev;
  a.seed = e->seed;
  a.gid_base = e->env_id_base;
  const dim3 grid((unsigned)a.N), block(c.mode == LM_MODE_STEP ? 256 : 64);
  if (a.tab_n)
    hipLaunchKernelGGL(metalm_kernel<true>, grid, block, sizeof(double) * (size_t)a.tab_n, e->stream, a, c);
  else
    hipLaunchKernelGGL(metalm_kernel<false>, grid, block, 0, e->stream, a, c);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_metalm_reset(xv_metalm* h, const double* u_query, int32_t* query, int32_t* query_len) {
  XV_CHECK_ARG(h != nullptr);
  LMCall c = LMCall();
  c.mode = LM_MODE_RESET;
  c.u[0] = u_query;
  c.out_tok[0] = query; c.out_len[0] = query_len; c.out_stride[0] = h->a.max_len;
  return lm_launch(h, __func__, c);
}

extern "C" int xv_metalm_policy(xv_metalm* h, const double* temperature, const double* u_policy, int32_t* answer,
                                int32_t* answer_len) {
  XV_CHECK_ARG(h != nullptr && temperature != nullptr && answer != nullptr && answer_len != nullptr);
  LMCall c = LMCall();
  c.mode = LM_MODE_POLICY;
  c.temp = temperature;
  c.u[0] = u_policy;
  c.out_tok[0] = answer; c.out_len[0] = answer_len; c.out_stride[0] = h->a.max_len;
  return lm_launch(h, __func__, c);
}

extern "C" int xv_metalm_step(xv_metalm* h, const int32_t* answer, const int32_t* answer_len, const uint8_t* cached,
                              const double* u_greedy, const double* u_low, const double* u_query, int32_t* query,
                              int32_t* query_len, double* reward, int32_t* steps, int32_t* label, double* ppl,
                              int32_t* greedy, int32_t* greedy_len, int32_t* low, int32_t* low_len) {
  XV_CHECK_ARG(h != nullptr && answer != nullptr && answer_len != nullptr && reward != nullptr);
  LMCall c = LMCall();
  c.mode = LM_MODE_STEP;
  c.ans = answer; c.ans_len = answer_len; c.cached = cached;
  c.u[1] = u_greedy; c.u[2] = u_low; c.u[3] = u_query;
  c.out_tok[0] = label; c.out_stride[0] = h->a.max_len + 1;
  c.out_tok[1] = greedy; c.out_len[1] = greedy_len; c.out_stride[1] = h->a.max_len;
  c.out_tok[2] = low; c.out_len[2] = low_len; c.out_stride[2] = h->a.max_len;
  c.out_tok[3] = query; c.out_len[3] = query_len; c.out_stride[3] = h->a.max_len;
  c.reward = reward; c.ppl = ppl; c.steps_out = steps;
  return lm_launch(h, __func__, c);
}

extern "C" int xv_metalm_stream(xv_metalm* h, int datatype, int L, int max_rounds, const double* t_choices, int n_choice,
                                const int32_t* t_index, const double* u_policy, const double* u_greedy, const double* u_low,
                                const double* u_query, const int32_t* marks, int32_t* data, int32_t* label, int32_t* filled,
                                int32_t* rounds, double* reward, int32_t* t_index_out) {
  XV_CHECK_ARG(h != nullptr && marks != nullptr && data != nullptr && label != nullptr && filled != nullptr &&
               rounds != nullptr);
  XV_CHECK_ARG(datatype == XV_METALM_QA || datatype == XV_METALM_QAR || datatype == XV_METALM_QARA);
  XV_CHECK_ARG(L >= 1 && L <= 0x3fffffff && max_rounds >= 1 && max_rounds <= 0x1fffffff);      // cursors and 2 K stay ints
  XV_CHECK_ARG(datatype == XV_METALM_QA || (t_choices != nullptr && n_choice >= 1));
  if (!h->task_set) {
    xv_set_error("%s: no task set (xv_metalm_set_task)", __func__);
    return XV_ERR_INVALID;
  }
  LMStream s = LMStream();
  for (int i = 0; i < 11; ++i) {
    XV_CHECK_ARG(marks[i] >= 0 && marks[i] < h->a.V);
    s.marks[i] = marks[i];
  }
  s.datatype = datatype; s.L = L; s.max_rounds = max_rounds;
  s.K = max_rounds * (datatype == XV_METALM_QARA ? 2 : 1);
  s.n_choice = n_choice; s.t_choices = t_choices; s.t_index = t_index;
  s.u[0] = u_policy; s.u[1] = u_greedy; s.u[2] = u_low; s.u[3] = u_query;
  s.data = data; s.label = label; s.filled = filled; s.rounds = rounds; s.reward = reward; s.t_index_out = t_index_out;
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  LMArgs a = h->a;
  const XvTickBind tb = xv_engine_bind_tick(e, 2 * (uint64_t)s.K);      // policy and step of every sub-step, used or not
  a.tick = tb.tick;
  a.tick_dev = tb.tick_dev;
  a.seed = e->seed;
  a.gid_base = e->env_id_base;
  const dim3 grid((unsigned)a.N), block(256);
  if (a.tab_n)
    hipLaunchKernelGGL(metalm_stream_kernel<true>, grid, block, sizeof(double) * (size_t)a.tab_n, e->stream, a, s);
  else
    hipLaunchKernelGGL(metalm_stream_kernel<false>, grid, block, 0, e->stream, a, s);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

static int lm_state_copy(xv_metalm* h, bool get, int32_t* query, int32_t* query_len, double* cache, int32_t* steps) {
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  const LMArgs& a = h->a;
  const size_t nq = sizeof(int32_t) * (size_t)a.N * a.max_len, nc = sizeof(double) * (size_t)a.N * a.H,
               ni = sizeof(int32_t) * (size_t)a.N;
  XV_HIP(hipMemcpyAsync(get ? (void*)query : a.query, get ? (void*)a.query : query, nq, hipMemcpyDeviceToDevice, e->stream));
  XV_HIP(hipMemcpyAsync(get ? (void*)query_len : a.query_len, get ? (void*)a.query_len : query_len, ni,
                        hipMemcpyDeviceToDevice, e->stream));
  XV_HIP(hipMemcpyAsync(get ? (void*)cache : a.cache, get ? (void*)a.cache : cache, nc, hipMemcpyDeviceToDevice, e->stream));
  XV_HIP(hipMemcpyAsync(get ? (void*)steps : a.steps, get ? (void*)a.steps : steps, ni, hipMemcpyDeviceToDevice, e->stream));
  return XV_OK;
}

extern "C" int xv_metalm_get_state(xv_metalm* h, int32_t* query, int32_t* query_len, double* cache, int32_t* steps) {
  XV_CHECK_ARG(h != nullptr && query && query_len && cache && steps);
  return lm_state_copy(h, true, query, query_len, cache, steps);
}

extern "C" int xv_metalm_set_state(xv_metalm* h, const int32_t* query, const int32_t* query_len, const double* cache,
                                   const int32_t* steps) {
  XV_CHECK_ARG(h != nullptr && query && query_len && cache && steps);
  return lm_state_copy(h, false, const_cast<int32_t*>(query), const_cast<int32_t*>(query_len), const_cast<double*>(cache),
                       const_cast<int32_t*>(steps));
}
#endif
