// anyhvac_sampler.hip — AnyHVAC tasks made on the device: xv_anyhvac_sample_tasks writes, per candidate, the float64 table
// row xv_anyhvac_set_task borrows (XV_ANYHVAC_TASK_DOUBLES) and an `extras` row with what the row does not keep (node
// locations, diffusion sigmas, the unification coefficient, the decision margins).
//
// Reference: xenoverse/anyhvac/anyhvac_sampler.py HVACTaskSampler, the node classes and wind_diffuser of
// anyhvac_utils.py, utils/random_nn.py RandomFourier; restated for numpy's stream in xenoverse_amd/anyhvac/task_sampler.py
// and, under this file's draws, in anyhvac/sampler_host.py, which the kernel is held to (exactly where only arithmetic is
// involved, within derived bounds where log / sin / cos / exp enter).
//
// One 256-lane workgroup is one candidate.  Phases: head scalars (every lane, redundantly) -> convection coefficients and
// heat capacities (lanes over walls and cells) -> placement by rejection (256 attempts per round, the lowest passing
// attempt wins through an LDS min) -> Fourier rows (a lane per node) -> unification keys and cooler rows (a lane per
// cooler) -> wind_diffuser as a fixed point (a wave per node, grid in LDS, whole-grid passes until no wave changes
// anything; numpy's pairwise order for the normalising sum) -> the week-long average heat (lanes over the 20,160 times,
// heaters in index order inside, a fixed tree over lanes).  Every loop has a bound that does not depend on the data.
// No cross-lane result depends on how work is dealt to lanes, and a candidate does not know its launch.
#include <climits>

#include "xv_common.h"
#include "xv_draws.h"

namespace {

constexpr int HS_T = 256, HS_WAVES = 4;
constexpr int HS_MAX_GRID = 16, HS_MAX_C = 320, HS_MAX_S = 640, HS_MAX_H = 640, HS_MAX_K = 16, HS_MAX_AMB = 4;
constexpr int HS_NODES = 640, HS_CELLS = HS_MAX_GRID * HS_MAX_GRID;
constexpr int HS_WALLS = (HS_MAX_GRID + 1) * (HS_MAX_GRID + 1) * 2;
constexpr int HS_PLACE_TRIES = 4096, HS_BIAS_TRIES = 256, HS_BIAS_SUB = 16, HS_HEATER_SUB = 128;
constexpr int HS_HEAT_TIMES = 20160, HS_HEAT_INTERVAL = 30;
constexpr double HS_COUNT_CAP = 1.0e6;
constexpr double HS_CUT = 1.0e-3, HS_MAX_POWER = 20000.0;
constexpr unsigned long long HS_INF_BITS = 0x7FF0000000000000ull;

enum : uint32_t { HS_P_HEAD = 0, HS_P_CHTC = 1, HS_P_HC = 2, HS_P_SENSOR_LOC = 3, HS_P_HEATER_LOC = 4, HS_P_COOLER_LOC = 5,
                  HS_P_SENSOR = 6, HS_P_BASE = 7, HS_P_HEATER = 8, HS_P_COOLER = 9, HS_P_UNIFY = 10 };
enum : int { HS_OK = 0, HS_PLACEMENT_CAP = 1, HS_UNIFY_EMPTY = 2, HS_TOO_BIG = 3 };

struct HsLds {
  double loc[HS_NODES][2];          // the kind being placed
  double hc[HS_CELLS];              // pitch NL
  double mat[HS_WAVES][HS_CELLS];   // a wave's diffuser grid, pitch nl (numpy's flat order)
  double wgt[HS_WAVES][16];         // exp(-d^2): source -> cells [0..3], source -> walls [4..7], centre -> cells, -> walls
  double red[HS_T];
  unsigned long long key[HS_MAX_C];
  unsigned long long margin[2];     // bias, diffuse: bits of a non-negative double
  uint16_t hcell[HS_NODES];         // a heater's cell, pitch NL
  uint8_t wall[HS_WALLS];           // pitch NL + 1
  uint8_t unified[HS_MAX_C];
  int win, bias_max;
};

struct HsArgs {
  uint64_t seed;
  int64_t cand_base;
  int n_cand, NW, NL, C, S, H, KS, KH;
  xv_anyhvac_sampler_params p;
  double* table;
  double* extras;
  xv_anyhvac_cand_info* info;
  int32_t* status;
};

struct HsRng {
  uint64_t seed, index;
};
__device__ __forceinline__ xv_u2 hs_pair(const HsRng& g, uint32_t purpose, uint32_t tick, uint32_t sub) {
  return xv_pair(xv_index_draw(g.seed, g.index, tick, purpose, sub));
}
// element q of a block of uniforms: half q & 1 of call q >> 1
__device__ __forceinline__ double hs_block(const HsRng& g, uint32_t purpose, uint32_t q) {
  const xv_u2 u = hs_pair(g, purpose, 0, q >> 1);
  return (q & 1u) ? u.b : u.a;
}
__device__ __forceinline__ double hs_uni(double u, const double r[2]) { return r[0] + (r[1] - r[0]) * u; }
// the reference's order of directions: (-1, 0), (0, -1), (1, 0), (0, 1)
__device__ __forceinline__ int hs_di(int d) { return d == 0 ? -1 : (d == 2 ? 1 : 0); }
__device__ __forceinline__ int hs_dj(int d) { return d == 1 ? -1 : (d == 3 ? 1 : 0); }
__device__ __forceinline__ int hs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct HsOff {
  int NC, NWALL, sens_row, heat_row;
  size_t base, chtc, hc, sens, heat, hd, cool, cd, cv, doubles;
  size_t e_sloc, e_hloc, e_cloc, e_hsig, e_csig, e_tail, extras;
};
__host__ __device__ inline HsOff hs_offsets(int NW, int NL, int C, int S, int H, int KS, int KH) {
  HsOff o;
  o.NC = NW * NL;
  o.NWALL = (NW + 1) * (NL + 1) * 2;
  o.sens_row = 8 + 3 * KS;
  o.heat_row = 4 + 3 * KH;
  o.base = 16;
  o.chtc = o.base + 3 * (size_t)KH;
  o.hc = o.chtc + o.NWALL;
  o.sens = o.hc + o.NC;
  o.heat = o.sens + (size_t)S * o.sens_row;
  o.hd = o.heat + (size_t)H * o.heat_row;
  o.cool = o.hd + (size_t)H * o.NC;
  o.cd = o.cool + (size_t)C * 24;
  o.cv = o.cd + (size_t)C * o.NC;
  o.doubles = o.cv + (size_t)C * o.NWALL;
  o.e_sloc = 0;
  o.e_hloc = 2 * (size_t)S;
  o.e_cloc = o.e_hloc + 2 * (size_t)H;
  o.e_hsig = o.e_cloc + 2 * (size_t)C;
  o.e_csig = o.e_hsig + H;
  o.e_tail = o.e_csig + C;      // unify coefficient, bias margin, diffuse margin, 0
  o.extras = o.e_tail + 4;
  return o;
}

// what tables.build_tables leaves where a task has nothing: heat capacity 1, periods 1, a cooler's delay 1, zeros
__device__ void hs_fill_padding(double* row, double* ex, const HsOff& o) {
  for (size_t i = threadIdx.x; i < o.doubles; i += HS_T) {
    double v = 0.0;
    if (i >= o.hc && i < o.sens) v = 1.0;
    else if (i >= o.sens && i < o.heat) v = ((i - o.sens) % (size_t)o.sens_row == 6) ? 1.0 : 0.0;
    else if (i >= o.heat && i < o.hd) v = ((i - o.heat) % (size_t)o.heat_row == 2) ? 1.0 : 0.0;
    else if (i >= o.cool && i < o.cd) v = ((i - o.cool) % 24 == 20) ? 1.0 : 0.0;
    row[i] = v;
  }
  for (size_t i = threadIdx.x; i < o.extras; i += HS_T)
    ex[i] = (i == o.e_tail + 1 || i == o.e_tail + 2) ? __longlong_as_double((long long)HS_INF_BITS) : 0.0;
}

// RandomFourier(ndim=1) from sub0: order / a / b rows (term 0 has order 0) -> the number of terms (<= max_item + 1)
__device__ int hs_fourier(const HsRng& g, uint32_t purpose, uint32_t tick, uint32_t sub0, int max_order, int max_item,
                          double box, double* order, double* ca, double* cb) {
  const int n_items = 1 + xv_floor_int(hs_pair(g, purpose, tick, sub0).a, max_item);
  const double scale = box / sqrt((double)n_items);
  for (int t = 0; t <= n_items; ++t) {
    const uint32_t b = sub0 + 1 + 4 * (uint32_t)t;
    double o = 0.0, zc, zs;
    if (t) {
      const int oi = 1 + xv_floor_int(hs_pair(g, purpose, tick, b).a, max_order);
      xv_normal2(hs_pair(g, purpose, tick, b + 1), &zc, &zs);
      o = (double)oi + zc;
    }
    xv_normal2(hs_pair(g, purpose, tick, b + 2), &zc, &zs);
    const xv_u2 e = hs_pair(g, purpose, tick, b + 3);
    order[t] = o;
    ca[t] = zc * (xv_expo(e.a) * scale);
    cb[t] = zs * (xv_expo(e.b) * scale);
  }
  return n_items + 1;
}

// a heat curve: (period, heat_base, n_terms) and its series
__device__ int hs_heat_curve(const HsRng& g, const xv_anyhvac_sampler_params& p, uint32_t purpose, uint32_t tick,
                             double* period, double* heat_base, double* order, double* ca, double* cb) {
  const xv_u2 u0 = hs_pair(g, purpose, tick, 0), u1 = hs_pair(g, purpose, tick, 1);
  const int lo = p.heat_period_lo * 60, hi = p.heat_period_hi * 60;
  *period = (double)((lo + xv_floor_int(u0.a, hi - lo)) * 60);
  const double scale = hs_uni(u0.b, p.range[XV_ANYHVAC_R_HEAT_SCALE]);
  *heat_base = hs_uni(u1.a, p.range[XV_ANYHVAC_R_HEAT_BASE]);
  return hs_fourier(g, purpose, tick, 2, p.heat_max_order, p.heat_max_item, scale, order, ca, cb);
}

// bilinear_setup of one node -> s0, s1, d0, d1, k0, k1 and the node's cell
__device__ __forceinline__ void hs_bilinear(double lx, double ly, double cs, int nw, int nl, double* out6, double* nloc2) {
  const double l[2] = {lx, ly};
  const int hi[2] = {nw - 1, nl - 1};
#pragma unroll
  for (int ax = 0; ax < 2; ++ax) {
    const double cloc = l[ax] / cs;
    const int n = (int)cloc;
    const double dloc = cloc - (double)n - 0.5;
    const double fl = floor(dloc);
    const int sg = (int)fl + n;
    out6[ax] = (double)hs_clamp(sg, 0, hi[ax]);
    out6[2 + ax] = (double)hs_clamp(sg + 1, 0, hi[ax]);
    out6[4 + ax] = dloc - fl;
    if (nloc2) nloc2[ax] = (double)n;
  }
}

// placement by rejection of n nodes into L.loc: attempt a of node i draws from (purpose, tick i, sub a); per round every
// lane tests one attempt against all earlier nodes, the lowest passing attempt wins.  false: a node found no place.
__device__ bool hs_place(HsLds& L, const HsRng& g, uint32_t purpose, int n, double dw, double dl, double cs, int nw, int nl,
                         double min_dist, int* place_max) {
  const int tid = threadIdx.x;
  const double idw = (double)(int)dw, md2 = min_dist * min_dist;
  for (int i = 0; i < n; ++i) {
    int w = INT_MAX;
    for (int r = 0; r < HS_PLACE_TRIES / HS_T; ++r) {
      if (tid == 0) L.win = INT_MAX;
      __syncthreads();
      const int a = r * HS_T + tid;
      const xv_u2 u = hs_pair(g, purpose, (uint32_t)i, (uint32_t)a);
      const double x = floor(u.a * idw), y = dl * u.b;
      bool ok = (x / cs < (double)nw) && (y / cs < (double)nl);      // the node's cell exists
      for (int j = 0; ok && j < i; ++j) {
        const double dx = L.loc[j][0] - x, dy = L.loc[j][1] - y;
        if (dx * dx + dy * dy < md2) ok = false;
      }
      if (ok) atomicMin(&L.win, a);
      __syncthreads();
      w = L.win;
      __syncthreads();
      if (w != INT_MAX) {
        if (a == w) {
          L.loc[i][0] = x;
          L.loc[i][1] = y;
        }
        break;
      }
    }
    if (w == INT_MAX) return false;
    *place_max = w + 1 > *place_max ? w + 1 : *place_max;
  }
  __syncthreads();
  return true;
}

// numpy's pairwise sum of n <= 256 contiguous doubles (csrc/anymdp_vi_host.hip np_sum)
__device__ double hs_sum_block(const double* a, int n) {      // n <= 128
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}
__device__ double hs_sum_split(const double* a, int n) {      // pieces of a split of n <= 256: one more split at most
  if (n <= 128) return hs_sum_block(a, n);
  int half = n / 2;
  half -= half % 8;
  return hs_sum_block(a, half) + hs_sum_block(a + half, n - half);
}
__device__ double hs_np_sum(const double* a, int n) {
  if (n <= 128) return hs_sum_block(a, n);
  int half = n / 2;
  half -= half % 8;
  return hs_sum_split(a, half) + hs_sum_split(a + half, n - half);
}

// one curve's power at time t: heat_base + the positive part of the series, capped
__device__ __forceinline__ double hs_curve_power(double heat_base, double period, int n, const double* order, const double* ca,
                                                 const double* cb, double t) {
  const double x = t / period;
  double y = 0.0;
  for (int j = 0; j < n; ++j) {
    const double ang = order[j] * x;
    y = y + (ca[j] * sin(ang) + cb[j] * cos(ang));
  }
  return fmin(heat_base + fmax(y, 0.0), HS_MAX_POWER);
}

__global__ __launch_bounds__(HS_T) void anyhvac_sampler_kernel(HsArgs P) {
  __shared__ HsLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cand = blockIdx.x;
  const xv_anyhvac_sampler_params& p = P.p;
  const HsRng g{P.seed, (uint64_t)(P.cand_base + cand)};
  const int NW = P.NW, NL = P.NL, KS = P.KS, KH = P.KH;
  const HsOff o = hs_offsets(NW, NL, P.C, P.S, P.H, KS, KH);
  double* row = P.table + (size_t)cand * o.doubles;
  double* ex = P.extras + (size_t)cand * o.extras;

  hs_fill_padding(row, ex, o);
  if (tid < 2) L.margin[tid] = HS_INF_BITS;
  if (tid == 0) L.bias_max = 0;
  __syncthreads();      // the padding is down before any lane writes a value over it

  // ---- 1. head scalars ----
  const xv_u2 h0 = hs_pair(g, HS_P_HEAD, 0, 0), h1 = hs_pair(g, HS_P_HEAD, 0, 1), h2 = hs_pair(g, HS_P_HEAD, 0, 2),
              h3 = hs_pair(g, HS_P_HEAD, 0, 3), h4 = hs_pair(g, HS_P_HEAD, 0, 4), h5 = hs_pair(g, HS_P_HEAD, 0, 5),
              h6 = hs_pair(g, HS_P_HEAD, 0, 6), h7 = hs_pair(g, HS_P_HEAD, 0, 7);
  const int nw = p.nw_lo + xv_floor_int(h0.a, p.nw_hi - p.nw_lo), nl = p.nl_lo + xv_floor_int(h0.b, p.nl_hi - p.nl_lo);
  const double cs = hs_uni(h1.a, p.range[XV_ANYHVAC_R_CELL_SIZE]);
  const double floor_height = hs_uni(h1.b, p.range[XV_ANYHVAC_R_FLOOR_HEIGHT]);
  const double dw = (double)nw * cs, dl = (double)nl * cs;
  const double area = dw * dl;
  const double cell_volume = floor_height * cs * cs;
  const double wall_chtc = hs_uni(h2.a, p.range[XV_ANYHVAC_R_WALL_CHTC]);
  const double floorceil_chtc = hs_uni(h2.b, p.range[XV_ANYHVAC_R_FLOOR_CHTC]);
  // (counts: capped at HS_COUNT_CAP before the conversion, far above any table: such a candidate is too_big)
  int nS = (int)fmin(area * hs_uni(h3.a, p.range[XV_ANYHVAC_R_SENSOR_DENSITY]), HS_COUNT_CAP);
  int nH = (int)fmin(area * hs_uni(h3.b, p.range[XV_ANYHVAC_R_HEATER_DENSITY]), HS_COUNT_CAP);
  int nC = (int)fmin(area * hs_uni(h4.a, p.range[XV_ANYHVAC_R_COOLER_DENSITY]), HS_COUNT_CAP);
  nS = nS < 1 ? 1 : nS;
  nH = nH < 1 ? 1 : nH;
  nC = nC < 1 ? 1 : nC;
  double wsum = 0.0;
  for (int q = 0; q < p.n_ambient; ++q) wsum = wsum + p.ambient_w[q];
  double eps = h4.b * wsum, t_b = p.ambient_low, ambient = 0.0;
  for (int q = 0; q < p.n_ambient; ++q) {
    if (eps < p.ambient_w[q] || q == p.n_ambient - 1) {
      ambient = t_b + (p.ambient_pt[q] - t_b) * h5.a;
      break;
    }
    eps -= p.ambient_w[q];
    t_b = p.ambient_pt[q];
  }
  const double target = p.has_target ? p.target : rint(hs_uni(h5.b, p.range[XV_ANYHVAC_R_TARGET]) * 2.0) / 2.0;
  const double drift_std = 1.0 + (2.0 - 1.0) * h6.a;
  const double sample_ratio = h6.b;

  int place_max = 0, passes = 0, n_unified = 0;
  int st = HS_OK;
  if (nw > NW || nl > NL || nC > P.C || nS > P.S || nH > P.H) st = HS_TOO_BIG;
  else if (nC == 1 && sample_ratio >= 0.4 && sample_ratio < 0.8) st = HS_UNIFY_EMPTY;

  const int ncell = nw * nl, nwall = (nw + 1) * (nl + 1) * 2;
  if (st == HS_OK) {
    // ---- 2. convection coefficients, heat capacities ----
    for (int q = tid; q < nwall; q += HS_T) {
      const int d = q & 1, i = (q >> 1) / (nl + 1), j = (q >> 1) % (nl + 1);
      double v = hs_uni(hs_block(g, HS_P_CHTC, (uint32_t)q), p.range[XV_ANYHVAC_R_INTERNAL_CHTC]);
      if ((d == 0 && (i == 0 || i == nw)) || (d == 1 && (j == 0 || j == nl))) v = wall_chtc;
      const int at = (i * (NL + 1) + j) * 2 + d;
      L.wall[at] = v < 5.0 ? 1 : 0;
      row[o.chtc + at] = v;
    }
    for (int q = tid; q < ncell; q += HS_T)
      L.hc[(q / nl) * NL + q % nl] = hs_uni(hs_block(g, HS_P_HC, (uint32_t)q), p.range[XV_ANYHVAC_R_GRID_HC]) * cell_volume;
    __syncthreads();

    // ---- 3. placement (and the bilinear reads of sensors and coolers) ----
    const double cooler_dist = cs < 2.0 ? cs : 2.0;
    if (!hs_place(L, g, HS_P_SENSOR_LOC, nS, dw, dl, cs, nw, nl, 1.2, &place_max)) st = HS_PLACEMENT_CAP;
    if (st == HS_OK) {
      for (int i = tid; i < nS; i += HS_T) {
        ex[o.e_sloc + 2 * i] = L.loc[i][0];
        ex[o.e_sloc + 2 * i + 1] = L.loc[i][1];
        hs_bilinear(L.loc[i][0], L.loc[i][1], cs, nw, nl, row + o.sens + (size_t)i * o.sens_row, nullptr);
      }
      __syncthreads();
      if (!hs_place(L, g, HS_P_HEATER_LOC, nH, dw, dl, cs, nw, nl, 1.2, &place_max)) st = HS_PLACEMENT_CAP;
    }
    if (st == HS_OK) {
      for (int i = tid; i < nH; i += HS_T) {
        ex[o.e_hloc + 2 * i] = L.loc[i][0];
        ex[o.e_hloc + 2 * i + 1] = L.loc[i][1];
        L.hcell[i] = (uint16_t)((int)(L.loc[i][0] / cs) * NL + (int)(L.loc[i][1] / cs));
      }
      __syncthreads();
      if (!hs_place(L, g, HS_P_COOLER_LOC, nC, dw, dl, cs, nw, nl, cooler_dist, &place_max)) st = HS_PLACEMENT_CAP;
    }
    if (st == HS_OK) {
      for (int i = tid; i < nC; i += HS_T) {
        double* r = row + o.cool + (size_t)i * 24;
        ex[o.e_cloc + 2 * i] = L.loc[i][0];
        ex[o.e_cloc + 2 * i + 1] = L.loc[i][1];
        hs_bilinear(L.loc[i][0], L.loc[i][1], cs, nw, nl, r, r + 6);
      }
    }
    __syncthreads();
    if (st != HS_OK) {      // the row goes back to all padding
      hs_fill_padding(row, ex, o);
    }
  }
  if (st != HS_OK) {
    if (tid == 0) {
      P.status[cand] = st;
      if (P.info) P.info[cand] = xv_anyhvac_cand_info{st, nw, nl, nC, nS, nH, place_max, 0, 0, 0};
    }
    return;
  }

  // ---- 4. Fourier rows: sensors, the base heater, heaters; equipment heat capacity in heater order ----
  for (int i = tid; i < nS; i += HS_T) {
    double* r = row + o.sens + (size_t)i * o.sens_row;
    const xv_u2 u = hs_pair(g, HS_P_SENSOR, (uint32_t)i, 0);
    const int lo = p.sensor_period_lo * 60, hi = p.sensor_period_hi * 60;
    r[6] = (double)(lo + xv_floor_int(u.a, hi - lo));
    const double box = fmin(xv_expo(u.b) * p.sensor_drift_mean, p.sensor_drift_ub);
    r[7] = (double)hs_fourier(g, HS_P_SENSOR, (uint32_t)i, 1, p.sensor_max_order, p.sensor_max_items, box, r + 8, r + 8 + KS,
                              r + 8 + 2 * KS);
  }
  if (tid == HS_T - 1) {
    double period, heat_base;
    const int n = hs_heat_curve(g, p, HS_P_BASE, 0, &period, &heat_base, row + o.base, row + o.base + KH, row + o.base + 2 * KH);
    row[11] = heat_base;
    row[12] = period;
    row[13] = (double)n;
  }
  for (int i = tid; i < nH; i += HS_T) {
    double* r = row + o.heat + (size_t)i * o.heat_row;
    double period, heat_base;
    const int n = hs_heat_curve(g, p, HS_P_HEATER, (uint32_t)i, &period, &heat_base, r + 4, r + 4 + KH, r + 4 + 2 * KH);
    const xv_u2 u = hs_pair(g, HS_P_HEATER, (uint32_t)i, HS_HEATER_SUB);
    ex[o.e_hsig + i] = hs_uni(u.a, p.range[XV_ANYHVAC_R_HEAT_SIGMA]);
    r[0] = hs_uni(u.b, p.range[XV_ANYHVAC_R_BASE_FACTOR]);
    r[1] = heat_base;
    r[2] = period;
    r[3] = (double)n;
  }
  for (int q = tid; q < ncell; q += HS_T) {
    const int at = (q / nl) * NL + q % nl;
    double v = L.hc[at];
    for (int i = 0; i < nH; ++i)
      if ((int)L.hcell[i] == at)
        v += hs_uni(hs_pair(g, HS_P_HEATER, (uint32_t)i, HS_HEATER_SUB + 1).a, p.range[XV_ANYHVAC_R_EQUIPMENT_HC]);
    row[o.hc + at] = v;
  }

  // ---- 5. unification keys, cooler rows ----
  const int mode = sample_ratio < 0.4 ? 1 : (sample_ratio < 0.8 ? 2 : 0);
  int n_to_unify = 0;
  if (mode == 2) {
    n_to_unify = (int)((double)(nC - 1) * (0.7 + (1.0 - 0.7) * h7.a));
    n_to_unify = n_to_unify < 1 ? 1 : n_to_unify;
  }
  n_unified = mode == 1 ? nC : n_to_unify;
  for (int q = tid; q < nC; q += HS_T) {
    const xv_u32x4 w = xv_index_draw(g.seed, g.index, 0, HS_P_UNIFY, (uint32_t)q >> 1);
    L.key[q] = (q & 1) ? xv_k53(w.z, w.w) : xv_k53(w.x, w.y);
  }
  __syncthreads();
  for (int q = tid; q < nC; q += HS_T) {
    int rank = 0;
    const unsigned long long k = L.key[q];
    for (int r = 1; r < nC; ++r) rank += (L.key[r] < k || (L.key[r] == k && r < q)) ? 1 : 0;
    L.unified[q] = (mode == 1 || (mode == 2 && q >= 1 && rank < n_to_unify)) ? 1 : 0;
  }
  __syncthreads();
  const double bound = fmin(32.0 - target - 2.0, 6.0);
  {
    double bmargin = __longlong_as_double((long long)HS_INF_BITS);
    int bias_max = 0;
    for (int i = tid; i < nC; i += HS_T) {
      double* r = row + o.cool + (size_t)i * 24;
      const uint32_t own = (uint32_t)i, shared = L.unified[i] ? 0u : (uint32_t)i;
      // what a unified cooler takes from cooler 0
      const xv_u2 s0 = hs_pair(g, HS_P_COOLER, shared, 0), s1 = hs_pair(g, HS_P_COOLER, shared, 1),
                  s2 = hs_pair(g, HS_P_COOLER, shared, 2), s4 = hs_pair(g, HS_P_COOLER, shared, 4),
                  s5 = hs_pair(g, HS_P_COOLER, shared, 5);
      r[8] = hs_uni(s0.a, p.range[XV_ANYHVAC_R_VENT_EFFICIENCY]);
      r[9] = hs_uni(s0.b, p.range[XV_ANYHVAC_R_EER_BASE]);
      r[10] = hs_uni(s1.a, p.range[XV_ANYHVAC_R_EER_DECAY_START]);
      r[11] = hs_uni(s1.b, p.range[XV_ANYHVAC_R_EER_ZERO_POINT]);
      r[12] = hs_uni(s2.a, p.range[XV_ANYHVAC_R_EER_REVERSE]);
      ex[o.e_csig + i] = hs_uni(s2.b, p.range[XV_ANYHVAC_R_COOLER_SIGMA]);
      r[15] = hs_uni(s4.a, p.range[XV_ANYHVAC_R_MAX_COOLING_POWER]);
      const double vent_min = hs_uni(s4.b, p.range[XV_ANYHVAC_R_POWER_VENT_MIN]);
      r[16] = vent_min;      // min_cooling_power: the first draw of power_vent_min
      if (s5.a < p.vent_fixed_factor) {
        r[18] = hs_uni(s5.b, p.range[XV_ANYHVAC_R_FIXED_RATIO]);
        r[17] = vent_min;
      } else {
        r[18] = 0.0;
        r[17] = hs_uni(s5.b, p.range[XV_ANYHVAC_R_FIXED_POWER]);
      }
      // its own
      const xv_u2 c3 = hs_pair(g, HS_P_COOLER, own, 3), c6 = hs_pair(g, HS_P_COOLER, own, 6);
      r[13] = hs_uni(c3.a, p.range[XV_ANYHVAC_R_DECAY_UB]);
      r[14] = hs_uni(c3.b, p.range[XV_ANYHVAC_R_DECAY_LB]);
      double sample = 0.0;
      for (int a = 0; a < HS_BIAS_TRIES; ++a) {
        double zc, zs;
        xv_normal2(hs_pair(g, HS_P_COOLER, own, (uint32_t)(HS_BIAS_SUB + a)), &zc, &zs);
        const double s = p.bias_mean + drift_std * zc;
        bmargin = fmin(bmargin, fabs(fabs(s) - bound) / bound);
        if (-bound <= s && s <= bound) {
          sample = s;
          bias_max = a + 1 > bias_max ? a + 1 : bias_max;
          break;
        }
      }
      r[19] = c6.a < p.sign_prob ? fabs(sample) : -fabs(sample);
      r[20] = hs_uni(c6.b, p.range[XV_ANYHVAC_R_DELAY]);
    }
    atomicMin(&L.margin[0], (unsigned long long)__double_as_longlong(bmargin));
    atomicMax(&L.bias_max, bias_max);
  }
  __syncthreads();      // locations and sigmas in `extras`, heater rows: visible to every lane from here

  // ---- 6. wind_diffuser as a fixed point: a wave per node, four nodes per round ----
  {
    double dmargin = __longlong_as_double((long long)HS_INF_BITS);
    const int n_nodes = nH + nC;
    for (int base = 0; base < n_nodes; base += HS_WAVES) {
      const int node = base + wave;
      const bool active = node < n_nodes, heater = node < nH;
      const int k = heater ? node : node - nH;
      double lx = 0.5, ly = 0.5, sigma = 1.0;
      if (active) {
        lx = ex[(heater ? o.e_hloc : o.e_cloc) + 2 * k];
        ly = ex[(heater ? o.e_hloc : o.e_cloc) + 2 * k + 1];
        sigma = ex[(heater ? o.e_hsig : o.e_csig) + k];
      }
      const double gx = lx / cs, gy = ly / cs;
      const int si = (int)gx, sj = (int)gy, src = si * nl + sj;
      if (lane < 16) {
        const int which = lane >> 2, d = lane & 3;
        const bool from_src = which < 2, to_wall = (which & 1) != 0;
        const double px = from_src ? gx : 0.5, py = from_src ? gy : 0.5;
        const int ci = from_src ? si : 0, cj = from_src ? sj : 0;
        const int ni = ci + hs_di(d), nj = cj + hs_dj(d);
        const double qx = to_wall ? (0.5 * (double)ni + 0.5 * (double)ci) : ((double)ni + 0.5);
        const double qy = to_wall ? (0.5 * (double)nj + 0.5 * (double)cj) : ((double)nj + 0.5);
        const double tx = (px - qx) * cs / sigma, ty = (py - qy) * cs / sigma;
        L.wgt[wave][lane] = exp(-(tx * tx + ty * ty));
      }
      for (int q = lane; q < ncell; q += 64) L.mat[wave][q] = (active && q == src) ? 1.0 : 0.0;
      __syncthreads();
      const double* W = L.wgt[wave];
      double* M = L.mat[wave];
      int pass = 0;
      for (; pass < ncell + 2; ++pass) {
        double nv[4];
        int changed = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int q = lane + 64 * s;
          nv[s] = 0.0;
          if (active && q < ncell) {
            const int i = q / nl, j = q % nl;
            const double cur = M[q];
            double best = cur;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const int ci = i - hs_di(d), cj = j - hs_dj(d);      // the cell that spreads to (i, j) in direction d
              if (ci < 0 || cj < 0 || ci >= nw || cj >= nl) continue;
              const int wi = ci + (hs_di(d) > 0 ? 1 : 0), wj = cj + (hs_dj(d) > 0 ? 1 : 0), w = hs_di(d) == 0 ? 1 : 0;
              if (L.wall[(wi * (NL + 1) + wj) * 2 + w]) continue;
              const int c = ci * nl + cj;
              const double mc = M[c];
              if (c == src || mc > HS_CUT) {
                const double kk = (c == src ? W[d] : W[8 + d]) * mc;
                best = kk > best ? kk : best;
              }
            }
            nv[s] = best;
            changed |= best != cur ? 1 : 0;
          }
        }
        const int any = __syncthreads_or(changed);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int q = lane + 64 * s;
          if (active && q < ncell) M[q] = nv[s];
        }
        __syncthreads();
        if (!any) break;
      }
      passes = pass + 1 > passes ? pass + 1 : passes;
      if (active) {
        for (int q = lane; q < ncell; q += 64) {
          const double v = M[q];
          if (v > 0.0 && q != src) dmargin = fmin(dmargin, fabs(v - HS_CUT) / HS_CUT);
        }
        if (!heater) {      // the wall matrix from the final cell values
          double* out = row + o.cv + (size_t)k * o.NWALL;
          for (int q = lane; q < nwall; q += 64) {
            const int d = q & 1, i = (q >> 1) / (nl + 1), j = (q >> 1) % (nl + 1);
            const int at = (i * (NL + 1) + j) * 2 + d;
            double v = 0.0;
            const bool inner = d == 0 ? (i >= 1 && i <= nw - 1 && j < nl) : (i < nw && j >= 1 && j <= nl - 1);
            if (inner && !L.wall[at]) {
              // the cell before the wall spreads in direction 2 (d = 0) or 3 (d = 1), the cell behind it in 0 or 1
              const int ca = d == 0 ? (i - 1) * nl + j : i * nl + (j - 1), cb = i * nl + j;
              const int da = d == 0 ? 2 : 3, db = d == 0 ? 0 : 1;
              const double ma = M[ca], mb = M[cb];
              if (ca == src || ma > HS_CUT) v = fmax(v, (ca == src ? W[4 + da] : W[12 + da]) * ma);
              if (cb == src || mb > HS_CUT) v = fmax(v, (cb == src ? W[4 + db] : W[12 + db]) * mb);
            }
            out[at] = v;
          }
        }
        if (lane == 0) L.red[wave] = hs_np_sum(M, ncell);
      }
      __syncthreads();
      if (active) {
        const double total = L.red[wave];
        double* out = row + (heater ? o.hd : o.cd) + (size_t)k * o.NC;
        for (int q = lane; q < ncell; q += 64) out[(q / nl) * NL + q % nl] = M[q] / total;
      }
      __syncthreads();
    }
    atomicMin(&L.margin[1], (unsigned long long)__double_as_longlong(dmargin));
  }

  // ---- 8. the week-long average heat ----
  double avg = 10000.0;
  if (!p.generate_task) {
    const double b_hb = row[11], b_per = row[12];
    const int b_n = (int)row[13];
    const double* b_o = row + o.base;
    double acc = 0.0;
    for (int kt = tid; kt < HS_HEAT_TIMES; kt += HS_T) {
      const double t = (double)(kt * HS_HEAT_INTERVAL);
      const double pb = hs_curve_power(b_hb, b_per, b_n, b_o, b_o + KH, b_o + 2 * KH, t);
      double step = 0.0;
      for (int h = 0; h < nH; ++h) {
        const double* r = row + o.heat + (size_t)h * o.heat_row;
        const double f = r[0];
        const double own = hs_curve_power(r[1], r[2], (int)r[3], r + 4, r + 4 + KH, r + 4 + 2 * KH, t);
        step = step + (f * pb + (1.0 - f) * own);
      }
      acc += step;
    }
    L.red[tid] = acc;
    __syncthreads();
    for (int s = HS_T / 2; s > 0; s >>= 1) {
      if (tid < s) L.red[tid] = L.red[tid] + L.red[tid + s];
      __syncthreads();
    }
    avg = L.red[0] / (double)HS_HEAT_TIMES;
  }
  __syncthreads();

  if (tid == 0) {
    row[0] = (double)nw; row[1] = (double)nl; row[2] = (double)nC; row[3] = (double)nS; row[4] = (double)nH;
    row[5] = cs; row[6] = floor_height; row[7] = floorceil_chtc; row[8] = ambient; row[9] = target; row[10] = avg;
    row[14] = (target - p.set_lower) / (p.set_upper - p.set_lower);
    row[15] = target + 6.0;
    ex[o.e_tail] = mode == 1 ? 1.0 : (mode == 2 ? (double)(n_to_unify + 1) / (double)nC : 0.0);
    ex[o.e_tail + 1] = __longlong_as_double((long long)L.margin[0]);
    ex[o.e_tail + 2] = __longlong_as_double((long long)L.margin[1]);
    P.status[cand] = HS_OK;
    if (P.info) P.info[cand] = xv_anyhvac_cand_info{HS_OK, nw, nl, nC, nS, nH, place_max, passes, n_unified, L.bias_max};
  }
}

bool hs_range_ok(const double r[2]) { return r[0] == r[0] && r[1] == r[1] && r[0] <= r[1]; }

}  // namespace

#ifndef XV_KERNELS_ONLY
// the argument checks of xv_anyhvac_sample_tasks: everything before the launch, no device needed
extern "C" int xv_anyhvac_sampler_check(int64_t cand_base, int n_cand, int NW, int NL, int C, int S, int H, int KS, int KH,
                                        const xv_anyhvac_sampler_params* p, const double* table, const double* extras,
                                        const int32_t* status) {
  XV_CHECK_ARG(p != nullptr && table != nullptr && extras != nullptr && status != nullptr);
  XV_CHECK_ARG(n_cand > 0 && cand_base >= 0);
  XV_CHECK_ARG(NW >= 1 && NW <= HS_MAX_GRID && NL >= 1 && NL <= HS_MAX_GRID);
  XV_CHECK_ARG(C >= 1 && C <= HS_MAX_C && S >= 1 && S <= HS_MAX_S && H >= 1 && H <= HS_MAX_H);
  XV_CHECK_ARG(KS >= 2 && KS <= HS_MAX_K && KH >= 2 && KH <= HS_MAX_K);
  // a node index is a counter tick, below 2^24: implied by the limits above today, and cannot fail; it stays so that
  // raising HS_MAX_* cannot silently shift node indices out of counter word 3 (purpose | tick << 8)
  XV_CHECK_ARG(C < (1 << 24) && S < (1 << 24) && H < (1 << 24));
  XV_CHECK_ARG(p->n_ambient >= 1 && p->n_ambient <= HS_MAX_AMB);
  XV_CHECK_ARG(p->nw_lo >= 1 && p->nw_lo < p->nw_hi && p->nl_lo >= 1 && p->nl_lo < p->nl_hi);
  XV_CHECK_ARG(p->sensor_max_items >= 1 && p->sensor_max_items + 1 == KS && p->heat_max_item >= 1 && p->heat_max_item + 1 == KH);
  XV_CHECK_ARG(p->sensor_max_order >= 1 && p->heat_max_order >= 1);
  XV_CHECK_ARG(p->sensor_period_lo >= 1 && p->sensor_period_lo < p->sensor_period_hi && p->sensor_period_hi <= (1 << 24));
  XV_CHECK_ARG(p->heat_period_lo >= 1 && p->heat_period_lo < p->heat_period_hi && p->heat_period_hi <= (1 << 18));
  for (int r = 0; r < XV_ANYHVAC_SAMPLER_RANGES; ++r) XV_CHECK_ARG(hs_range_ok(p->range[r]));
  XV_CHECK_ARG(p->range[XV_ANYHVAC_R_CELL_SIZE][0] > 0 && (double)p->nw_lo * p->range[XV_ANYHVAC_R_CELL_SIZE][0] >= 1.0);
  XV_CHECK_ARG(p->range[XV_ANYHVAC_R_HEAT_SIGMA][0] > 0 && p->range[XV_ANYHVAC_R_COOLER_SIGMA][0] > 0);
  XV_CHECK_ARG(p->range[XV_ANYHVAC_R_SENSOR_DENSITY][0] >= 0 && p->range[XV_ANYHVAC_R_HEATER_DENSITY][0] >= 0 &&
               p->range[XV_ANYHVAC_R_COOLER_DENSITY][0] >= 0);
  // the cooler bias is drawn within +-min(32 - target - 2, 6): that bound must stay at or above 1
  XV_CHECK_ARG(32.0 - (p->has_target ? p->target : p->range[XV_ANYHVAC_R_TARGET][1]) - 2.0 >= 1.0);
  XV_CHECK_ARG(p->set_upper > p->set_lower);
  XV_CHECK_ARG(p->sensor_drift_mean > 0 && p->sensor_drift_ub > 0);
  for (int q = 0; q < p->n_ambient; ++q) XV_CHECK_ARG(p->ambient_w[q] > 0 && p->ambient_pt[q] == p->ambient_pt[q]);
  return XV_OK;
}

extern "C" int xv_anyhvac_sample_tasks(xv_engine* e, uint64_t seed, int64_t cand_base, int n_cand, int NW, int NL, int C, int S,
                                       int H, int KS, int KH, const xv_anyhvac_sampler_params* params, double* table,
                                       double* extras, xv_anyhvac_cand_info* info, int32_t* status) {
  XV_CHECK_ARG(e != nullptr);
  const int rc = xv_anyhvac_sampler_check(cand_base, n_cand, NW, NL, C, S, H, KS, KH, params, table, extras, status);
  if (rc != XV_OK) return rc;
  XV_HIP(hipSetDevice(e->device));
  HsArgs P{seed, cand_base, n_cand, NW, NL, C, S, H, KS, KH, *params, table, extras, info, status};
  hipLaunchKernelGGL(anyhvac_sampler_kernel, dim3(n_cand), dim3(HS_T), 0, e->stream, P);
  XV_LAUNCH_CHECK();
  return XV_OK;
}
#endif
