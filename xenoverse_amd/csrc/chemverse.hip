// chemverse.hip — ChemVerse on the device: the reference's chain-reaction simulator (xenoverse/chemverse/environment/
// simulator.py simulate_chain_reaction :639-880 and what it calls, :34-500, :614-636) for N independent experiments in one
// launch, each under its own world.  Host restatement and the full statement of the semantics: xenoverse_amd/chemverse/
// host.py; the tables: xenoverse_amd/chemverse/tables.py.  fp64 throughout; the library is built with -ffp-contract=off and
// no product-sum below is meant to be fused.
//
// Mapping: one lane per experiment, one 64-lane workgroup per 64 consecutive experiments, which the caller has grouped so
// that they belong to ONE world (exp_world < 0 marks a padding lane).  An experiment is serial and branchy — steps ->
// reactions -> Brent iterations — so throughput comes from the batch's width, not from cooperation inside an experiment; no
// lane ever waits for another: no atomics but the error word, no hand-offs, no spin waits, and one barrier (behind the
// staging of the world's per-chemical table).
//   LDS (dynamic, c_stride * 640 bytes: 40 KiB at the limit of 64 chemicals)
//     pool   double [chemical][lane]   the pool, 0 for a chemical that is not in it: a wave's access to one chemical, and a
//                                      gather through the order list, touch 64 distinct bank pairs (address = (c * 64 + lane) * 8)
//     order  uint8  [slot][lane]       the pool dict's insertion order (the reference iterates the dict: heat capacity, gas
//                                      moles, phase heat, the external-solvent search and gas loss sum in this order)
//     chem   double [8][chemical]      the world's per-chemical table
//   global workspace of the handle, [workgroup][array][chemical][lane] (coalesced), zeroed by the kernel itself:
//     step consumed / produced / byproduct, total consumed / produced / byproduct, gas lost; fired int32 [reaction][lane]
//   Reaction tables, solubility and equipment are read from global memory: a reaction's row is indexed by the loop counter
//   alone, the same for the whole wave (scalar loads); solubility is read only for an external solvent.
// Every loop has a bound known at launch: steps <= XV_CHEM_STEPS_MAX, reactions <= R, Brent <= 200 iterations (then the
// reference's fallback, half the largest extent), species <= C.
//
// Against the reference: exp, log and pow are the device library's (documented at 1-2 ulp) where the reference has numpy's
// and libm's, `x ** 0.5` is sqrt, an integer power is a product for 1 and 2; the sums run in the reference's order.  A Python
// OverflowError inside the objective (which the reference turns into half the largest extent) has no counterpart: the value
// is inf here.
#include "xv_common.h"

#define CHEM_LANES 64
#define CHEM_F 8       // columns of chem_f: mw, mp, bp, clausius_C, cp, latent fusion, latent vaporisation, is_solvent
#define CHEM_RXN_I 36  // columns of rxn_i: n_reactant, n_product, n_byproduct, n_catalyst, reactant[6], coeff[6], product[4],
                       // coeff[4], byproduct[4], coeff[4], catalyst[4]
#define CHEM_NR XV_CHEM_REACTANTS_MAX
#define CHEM_NP XV_CHEM_PRODUCTS_MAX
#define CHEM_NB XV_CHEM_BYPRODUCTS_MAX
#define CHEM_NC XV_CHEM_CATALYSTS_MAX
#define CHEM_ACC 7     // workspace arrays per workgroup
#define CHEM_SOLV_NONE (-1)
#define CHEM_SOLV_SELF (-2)
#define CHEM_SOLV_NEAT (-3)

struct ChemWorlds {
  const int32_t* world_off;   // [n_world + 1][4]: first chemical, reaction, equipment, solubility entry
  const double* chem_f;       // [sum C][8]
  const uint8_t* sol_present; // [sum C^2]: [chemical][solvent]
  const double* sol_value;
  const int32_t* rxn_i;       // [sum R][36]
  const double* rxn_f;        // [sum R][4]: delta_G_kJ, delta_H_kJ, activation_energy_kJ, log_A_factor
  const int64_t* rxn_solv;    // [sum R]: bit s = every non-solvent reactant lists solvent s
  const int32_t* eq_i;        // [sum E][2]: sealed, thermal mode
  const double* eq_f;         // [sum E][6]: max T, min T, max P, heat transfer coeff, max heat rate W, gas retention
  int n_world, c_stride, r_stride;
};

struct ChemExp {
  const int32_t* exp_world;
  const double* amounts;      // [n][c_stride]
  const int32_t* order;       // [n][c_stride]
  const int32_t* n_initial;
  const double *T, *P, *duration;
  const int32_t* equipment;
  const double *heating_rate, *volume;
  double step_seconds;
  int n_exp;
};

struct ChemOut {
  double *final_pool, *consumed, *produced, *byproduct, *gas_lost;
  int32_t* fired;
  int32_t *num_steps, *steps_run;
  uint8_t *converged, *failure;
  int32_t* failure_step;
  double *final_T, *final_P;
  int32_t* hist_step;
  double *hist_T, *hist_P;
  int32_t* hist_count;
  int32_t *log_step, *log_active;
  double *log_T, *log_P, *log_consumed, *log_produced;
  int32_t* log_count;
};

__device__ __forceinline__ double chem_clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

__device__ __forceinline__ double chem_powi(double c, int k) { return k == 1 ? c : (k == 2 ? c * c : pow(c, (double)k)); }

// solve_equilibrium_extent's objective (:183-190)
__device__ __forceinline__ double chem_objective(double xi, double K, const double (&r_mol)[CHEM_NR], const int (&r_k)[CHEM_NR],
                                                 int nr, const double (&p_mol)[CHEM_NP], const int (&p_k)[CHEM_NP], int np) {
  double num = 1.0, den = 1.0;
  bool bad = false, first = true;
#pragma unroll
  for (int j = 0; j < CHEM_NP; ++j)
    if (j < np) {
      const double c = p_mol[j] + (double)p_k[j] * xi;
      bad |= c < 0.0;
      const double t = chem_powi(c, p_k[j]);
      num = first ? t : num * t;
      first = false;
    }
  first = true;
#pragma unroll
  for (int j = 0; j < CHEM_NR; ++j)
    if (j < nr) {
      const double c = r_mol[j] - (double)r_k[j] * xi;
      bad |= c <= 0.0;
      const double t = chem_powi(c, r_k[j]);
      den = first ? t : den * t;
      first = false;
    }
  if (bad) return INFINITY;
  return num / den - K;
}

// scipy.optimize.brentq(xtol = 1e-10, rtol = 4 eps, maxiter = 200), step for step (host.py brentq_host); fa = f(0), fb =
// f(xb) of opposite signs.  *ok = false where scipy raises: a NaN value, or no convergence.
__device__ __forceinline__ double chem_brentq(double xb, double fa, double fb, double K, const double (&r_mol)[CHEM_NR],
                                              const int (&r_k)[CHEM_NR], int nr, const double (&p_mol)[CHEM_NP],
                                              const int (&p_k)[CHEM_NP], int np, bool* ok) {
  const double xtol = 1e-10, rtol = 8.881784197001252e-16;
  double xpre = 0.0, xcur = xb, xblk = 0.0, fpre = fa, fcur = fb, fblk = 0.0, spre = 0.0, scur = 0.0;
  *ok = true;
  if (fpre == 0.0) return xpre;
  if (fcur == 0.0) return xcur;
  for (int it = 0; it < 200; ++it) {
    if (fpre != 0.0 && fcur != 0.0 && (signbit(fpre) != signbit(fcur))) {
      xblk = xpre;
      fblk = fpre;
      spre = scur = xcur - xpre;
    }
    if (fabs(fblk) < fabs(fcur)) {
      xpre = xcur; xcur = xblk; xblk = xpre;
      fpre = fcur; fcur = fblk; fblk = fpre;
    }
    const double delta = (xtol + rtol * fabs(xcur)) / 2.0;
    const double sbis = (xblk - xcur) / 2.0;
    if (fcur == 0.0 || fabs(sbis) < delta) return xcur;
    if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
      double stry;
      if (xpre == xblk) {
        stry = -fcur * (xcur - xpre) / (fcur - fpre);
      } else {
        const double dpre = (fpre - fcur) / (xpre - xcur);
        const double dblk = (fblk - fcur) / (xblk - xcur);
        stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
      }
      if (2.0 * fabs(stry) < fmin(fabs(spre), 3.0 * fabs(sbis) - delta)) {
        spre = scur;
        scur = stry;
      } else {
        spre = sbis;
        scur = sbis;
      }
    } else {
      spre = sbis;
      scur = sbis;
    }
    xpre = xcur;
    fpre = fcur;
    if (fabs(scur) > delta) xcur += scur;
    else xcur += (sbis > 0.0 ? delta : -delta);
    fcur = chem_objective(xcur, K, r_mol, r_k, nr, p_mol, p_k, np);
    if (fcur != fcur) { *ok = false; return xcur; }
  }
  *ok = false;
  return xcur;
}

struct ChemLane {      // what the per-lane helpers need
  double* pool;        // + lane: element c at pool[c * 64]
  uint8_t* order;      // + lane: slot i at order[i * 64]
  const double* chem;  // [8][cs]
  int cs, C, n_order;
  double T, logP;      // logP = log(max(0.01, P))
};

// a chemical index / a count read from a reaction's row, kept inside the world / the row whatever the table holds
__device__ __forceinline__ int chem_ix(const int32_t* __restrict__ ri, int k, int C) {
  const int c = ri[k];
  return (unsigned)c < (unsigned)C ? c : 0;
}
__device__ __forceinline__ int chem_cnt(const int32_t* __restrict__ ri, int k, int most) {
  const int n = ri[k];
  return n < 0 ? 0 : (n > most ? most : n);
}

#define CHEM_POOL(L, c) ((L).pool[(c) * CHEM_LANES])
#define CHEM_PROP(L, k, c) ((L).chem[(k) * (L).cs + (c)])

__device__ __forceinline__ int chem_state(const ChemLane& L, int c) {      // state_at :34-41: 0 solid, 1 liquid, 2 gas
  if (L.T < CHEM_PROP(L, 1, c)) return 0;
  const double bp_adj = CHEM_PROP(L, 2, c) + CHEM_PROP(L, 3, c) * L.logP;
  return L.T < bp_adj ? 1 : 2;
}

// _find_common_solvent :219-278
__device__ __forceinline__ int chem_find_solvent(const ChemLane& L, const int32_t* __restrict__ ri, uint64_t solv_mask) {
  const int nr = chem_cnt(ri, 0, CHEM_NR);
  bool any_non = false, solid_or_gas = false;
  uint64_t reactants = 0ull;
  for (int j = 0; j < nr; ++j) {
    const int c = chem_ix(ri, 4 + j, L.C);
    reactants |= 1ull << c;
    if (CHEM_PROP(L, 7, c) == 0.0) {
      any_non = true;
      if (chem_state(L, c) != 1) solid_or_gas = true;
    }
  }
  if (!any_non) return CHEM_SOLV_SELF;
  for (int j = 0; j < nr; ++j) {
    const int c = chem_ix(ri, 4 + j, L.C);
    if (CHEM_PROP(L, 7, c) != 0.0 && ((solv_mask >> c) & 1ull) && chem_state(L, c) == 1) return c;
  }
  for (int i = 0; i < L.n_order; ++i) {
    const int s = L.order[i * CHEM_LANES];
    if (CHEM_POOL(L, s) > 1e-9 && CHEM_PROP(L, 7, s) != 0.0 && !((reactants >> s) & 1ull) && ((solv_mask >> s) & 1ull) &&
        chem_state(L, s) == 1)
      return s;
  }
  return solid_or_gas ? CHEM_SOLV_NONE : CHEM_SOLV_NEAT;
}

__device__ __forceinline__ double chem_heat_capacity(const ChemLane& L) {      // :57-65
  double total = 0.0;
  for (int i = 0; i < L.n_order; ++i) {
    const int c = L.order[i * CHEM_LANES];
    const double g = CHEM_POOL(L, c);
    if (g > 1e-9) total += g * CHEM_PROP(L, 4, c);
  }
  return fmax(total, 0.1);
}

__device__ __forceinline__ double chem_gas_moles(const ChemLane& L) {      // :68-80, at L.T, L.logP
  double total = 0.0;
  for (int i = 0; i < L.n_order; ++i) {
    const int c = L.order[i * CHEM_LANES];
    const double g = CHEM_POOL(L, c);
    if (g > 1e-9 && chem_state(L, c) == 2) total += g / CHEM_PROP(L, 0, c);
  }
  return total;
}

__device__ __forceinline__ double chem_phase_heat(const ChemLane& L, double old_T, double new_T) {      // :83-108
  double heat = 0.0;
  for (int i = 0; i < L.n_order; ++i) {
    const int c = L.order[i * CHEM_LANES];
    const double g = CHEM_POOL(L, c);
    if (g < 1e-9) continue;
    const double bp_adj = CHEM_PROP(L, 2, c) + CHEM_PROP(L, 3, c) * L.logP;
    const double mp = CHEM_PROP(L, 1, c);
    if (old_T < mp && mp <= new_T) heat += g * CHEM_PROP(L, 5, c);
    else if (new_T < mp && mp <= old_T) heat -= g * CHEM_PROP(L, 5, c);
    if (old_T < bp_adj && bp_adj <= new_T) heat += g * CHEM_PROP(L, 6, c);
    else if (new_T < bp_adj && bp_adj <= old_T) heat -= g * CHEM_PROP(L, 6, c);
  }
  return heat;
}

// ---- one experiment, in the pieces the simulator kernel and the cost oracle's kernel (chemverse_optimal.hip) share ----------
struct ChemWorldAt {      // a world's place in the concatenated tables
  int c0, r0, e0, s0, C, R, E;
};

// the workgroup's world wb: its offsets and sizes, kept inside the strides (else *err is set on lane 0), and its
// per-chemical table staged into s_chem.  Holds the one barrier: every lane of the workgroup calls it.
__device__ __forceinline__ ChemWorldAt chem_stage_world(const ChemWorlds& W, int wb, int lane, double* s_chem, uint32_t* err) {
  const int cs = W.c_stride, rs = W.r_stride;
  const int32_t* wo = W.world_off + 4 * wb;
  ChemWorldAt A;
  A.c0 = wo[0]; A.r0 = wo[1]; A.e0 = wo[2]; A.s0 = wo[3];
  int C = wo[4] - A.c0, R = wo[5] - A.r0, E = wo[6] - A.e0;
  if (C < 1 || C > cs || C > XV_CHEM_C_MAX || R < 0 || R > rs || E < 1) {
    if (lane == 0) *err |= XV_DEVERR_ACTION_RANGE;
    C = C < 1 ? 1 : (C > cs ? cs : C);
    if (C > XV_CHEM_C_MAX) C = XV_CHEM_C_MAX;
    R = R < 0 ? 0 : (R > rs ? rs : R);
    if (E < 1) E = 1;
  }
  A.C = C; A.R = R; A.E = E;
  for (int i = lane; i < CHEM_F * cs; i += CHEM_LANES) {
    const int k = i / cs, c = i - k * cs;
    s_chem[i] = c < C ? W.chem_f[(size_t)(A.c0 + c) * CHEM_F + k] : 0.0;
  }
  __syncthreads();
  return A;
}

#define CHEM_ACCUM(a, c) acc[((size_t)(a) * cs + (c)) * CHEM_LANES]      // of the names acc and cs where it is used

// an empty pool and zeroed accumulators
__device__ __forceinline__ void chem_lane_clear(ChemLane& L, uint64_t* member, double* acc, int32_t* fired, int R) {
  const int cs = L.cs;
  L.n_order = 0;
  *member = 0ull;
  for (int c = 0; c < L.C; ++c) {
    CHEM_POOL(L, c) = 0.0;
#pragma unroll
    for (int a = 0; a < CHEM_ACC; ++a) CHEM_ACCUM(a, c) = 0.0;
  }
  for (int r = 0; r < R; ++r) fired[r * CHEM_LANES] = 0;
}

// one entry of the initial amounts (:668-671): c is inside the world, g finite
__device__ __forceinline__ void chem_lane_charge(ChemLane& L, uint64_t* member, int c, double g) {
  if (((*member >> c) & 1ull) || !(g > 1e-9)) return;
  CHEM_POOL(L, c) = g;
  L.order[L.n_order * CHEM_LANES] = (uint8_t)c;
  ++L.n_order;
  *member |= 1ull << c;
}

struct ChemRun {      // in: the conditions; out: the run's scalars (T, P become the final ones)
  double T, P, duration, rate, volume;
  int eq;
  int num_steps, steps_run, failure, failure_step, converged_steps, hist_count, log_count;
};

// simulate_chain_reaction :673-843 for the charged lane.  The totals are left in the accumulators 3..6 and the pool in L;
// history and log rows go to O at experiment e where O has them.
__device__ __forceinline__ void chem_lane_run(const ChemWorlds& W, const ChemWorldAt& A, ChemLane& L, uint64_t member,
                                              double* acc, int32_t* fired, double step_seconds, ChemRun& X, const ChemOut& O,
                                              int e, uint32_t* errp) {
  const int cs = L.cs, C = A.C, R = A.R, r0 = A.r0, e0 = A.e0, s0 = A.s0;
  uint32_t err = 0u;
  double T = X.T, P = X.P;
  const double duration = X.duration, rate = X.rate, volume = X.volume;
  if (!(isfinite(T) && isfinite(P) && isfinite(duration) && isfinite(rate) && isfinite(volume))) err |= XV_DEVERR_NONFINITE;
  int eq = X.eq;
  if ((unsigned)eq >= (unsigned)A.E) { err |= XV_DEVERR_ACTION_RANGE; eq = 0; }
  const int sealed = W.eq_i[(size_t)(e0 + eq) * 2], mode = W.eq_i[(size_t)(e0 + eq) * 2 + 1];
  const double* ef = W.eq_f + (size_t)(e0 + eq) * 6;
  const double max_T = ef[0], min_T = ef[1], max_P = ef[2], htc = ef[3], max_heat_W = ef[4], retention = ef[5];
  const double T_init = T, P_init = P;

  L.T = T;
  L.logP = log(fmax(0.01, P));
  const double initial_gas_moles = chem_gas_moles(L);

  double steps_f = ceil(duration / step_seconds);      // :683-684
  int num_steps = steps_f >= 1.0 ? (steps_f <= (double)XV_CHEM_STEPS_MAX ? (int)steps_f : XV_CHEM_STEPS_MAX + 1) : 1;
  if (num_steps > XV_CHEM_STEPS_MAX) { err |= XV_DEVERR_ACTION_RANGE; num_steps = XV_CHEM_STEPS_MAX; }
  const double dt = duration / (double)num_steps;
  const int stride = num_steps / 20 > 1 ? num_steps / 20 : 1;

  int failure = 0, failure_step = -1, steps_run = 0, converged_steps = 0, hist_count = 0, log_count = 0;
  if (T > max_T || T < min_T) failure = 1;      // :689-716
  else if (P > max_P) failure = 2;

  for (int step = 0; step < num_steps && failure == 0; ++step) {
    steps_run = step + 1;
    // the applicable set, from the pool at the step's start (:308-335)
    uint64_t app[2] = {0ull, 0ull};
    int n_app = 0;
    for (int r = 0; r < R; ++r) {
      const int32_t* ri = W.rxn_i + (size_t)(r0 + r) * CHEM_RXN_I;
      const int nr = chem_cnt(ri, 0, CHEM_NR), nc = chem_cnt(ri, 3, CHEM_NC);
      bool have = true;
      for (int j = 0; j < nr; ++j) have = have && CHEM_POOL(L, chem_ix(ri, 4 + j, L.C)) > 1e-9;
      for (int j = 0; j < nc; ++j) have = have && CHEM_POOL(L, chem_ix(ri, 32 + j, L.C)) > 1e-9;
      if (have && chem_find_solvent(L, ri, (uint64_t)W.rxn_solv[r0 + r]) != CHEM_SOLV_NONE) {
        if (r < 64) app[0] |= 1ull << r; else app[1] |= 1ull << (r - 64);
        ++n_app;
      }
    }
    if (n_app == 0) {      // :725-729: no vessel update, no gas loss
      if (++converged_steps >= 3) break;
      continue;
    }
    double step_heat = 0.0;
    bool progress = false;
    for (int r = 0; r < R; ++r) {
      if (!(((r < 64 ? app[0] >> r : app[1] >> (r - 64))) & 1ull)) continue;
      const int32_t* ri = W.rxn_i + (size_t)(r0 + r) * CHEM_RXN_I;
      const double* rf = W.rxn_f + (size_t)(r0 + r) * 4;
      const int nr = chem_cnt(ri, 0, CHEM_NR), np = chem_cnt(ri, 1, CHEM_NP), nb = chem_cnt(ri, 2, CHEM_NB),
                nc = chem_cnt(ri, 3, CHEM_NC);
      const int solvent = chem_find_solvent(L, ri, (uint64_t)W.rxn_solv[r0 + r]);
      // _step_single_reaction :338-428
      const double T_K = T + 273.15;
      const double K_ref = exp(-rf[0] / (8.314e-3 * 298.0));
      const double K_eq = fmax(K_ref * exp(-rf[1] / 8.314e-3 * (1.0 / T_K - 1.0 / 298.0)), 1e-30);
      const double k_rate = pow(10.0, rf[3]) * exp(-rf[2] / (8.314e-3 * T_K));
      // phase factor :152-167 and heterogeneous factor :111-149
      double log_sum = 0.0, solid_mass = 0.0, gas_mass = 0.0, reactant_g = 0.0;
      int phases = 0;
      uint64_t reactants = 0ull;
      for (int j = 0; j < nr; ++j) {
        const int c = chem_ix(ri, 4 + j, L.C);
        reactants |= 1ull << c;
        const int st = chem_state(L, c);
        const double lf = log((st == 0 ? 0.01 : (st == 1 ? 1.0 : 8.0)) + 1e-30);
        log_sum = j == 0 ? lf : log_sum + lf;
        const double g = CHEM_POOL(L, c);
        reactant_g += g;
        if (g > 1e-9) {
          phases |= 1 << st;
          if (st == 0) solid_mass += g;
          if (st == 2) gas_mass += g;
        }
      }
      const double pf = exp(log_sum / (double)nr);
      double hetero = 1.0;
      if (__popc(phases) > 1) {
        if ((phases & 3) == 3) hetero *= fmax(0.01, pow(solid_mass, 2.0 / 3.0) / fmax(solid_mass, 0.1));
        if ((phases & 6) == 6) hetero *= fmin(1.0, P * 0.5) * fmax(0.05, sqrt(gas_mass) / fmax(gas_mass, 0.1));
        if ((phases & 5) == 5) hetero *= 0.05 * pow(P, 0.3);
        hetero = chem_clip(hetero, 0.001, 2.0);
      }
      double diss = 1.0;
      if (solvent == CHEM_SOLV_NEAT) diss = 0.3;
      else if (solvent >= 0 && !((reactants >> solvent) & 1ull)) {      // an external solvent: _dissolved_fraction :281-305
        const double solvent_g = CHEM_POOL(L, solvent);
        for (int j = 0; j < nr; ++j) {
          const int c = chem_ix(ri, 4 + j, L.C);
          double frac = 1.0;
          if (CHEM_PROP(L, 7, c) == 0.0) {
            const size_t si = (size_t)s0 + (size_t)c * C + solvent;
            const double v = W.sol_present[si] ? W.sol_value[si] : 0.0;
            const double cg = CHEM_POOL(L, c);
            if (v <= 0.0 || solvent_g < 1e-9 || cg <= 0.0) frac = 0.0;
            else frac = fmin(1.0, v * (solvent_g / 0.9 / 100.0) / cg);
          }
          diss = fmin(diss, frac);
        }
      }
      double cat_sum = 0.0;
      int n_cat = 0;
      for (int j = 0; j < nc; ++j) {
        const double g = CHEM_POOL(L, chem_ix(ri, 32 + j, L.C));
        if (g > 1e-9) { cat_sum += g; ++n_cat; }
      }
      double cat_factor = 1.0;
      if (n_cat > 0 && reactant_g > 0.0) cat_factor = 1.0 + 10.0 * sqrt(cat_sum / reactant_g);      // :208-216
      const double k_eff = k_rate * pf * hetero * cat_factor * diss;

      double r_mol[CHEM_NR], p_mol[CHEM_NP];
      int r_k[CHEM_NR], p_k[CHEM_NP];
      double max_extent = 0.0;
#pragma unroll
      for (int j = 0; j < CHEM_NR; ++j) {
        r_mol[j] = 0.0;
        r_k[j] = 1;
        if (j < nr) {
          const int c = chem_ix(ri, 4 + j, L.C);
          r_k[j] = ri[10 + j];
          r_mol[j] = CHEM_POOL(L, c) / CHEM_PROP(L, 0, c) * diss;
          const double q = r_mol[j] / (double)r_k[j];
          max_extent = (j == 0 || q < max_extent) ? q : max_extent;
        }
      }
#pragma unroll
      for (int j = 0; j < CHEM_NP; ++j) {
        p_mol[j] = 0.0;
        p_k[j] = 1;
        if (j < np) {
          const int c = chem_ix(ri, 16 + j, L.C);
          p_k[j] = ri[20 + j];
          p_mol[j] = CHEM_POOL(L, c) / CHEM_PROP(L, 0, c);
        }
      }
      max_extent *= 0.9999;
      double xi_eq = 0.0;      // solve_equilibrium_extent :170-205
      if (max_extent > 0.0) {
        const double f0 = chem_objective(0.0, K_eq, r_mol, r_k, nr, p_mol, p_k, np);
        const double f1 = chem_objective(max_extent, K_eq, r_mol, r_k, nr, p_mol, p_k, np);
        if (f0 * f1 < 0.0) {
          bool ok;
          xi_eq = chem_brentq(max_extent, f0, f1, K_eq, r_mol, r_k, nr, p_mol, p_k, np, &ok);
          if (!ok) xi_eq = max_extent * 0.5;
        } else if (f0 >= 0.0) {
          xi_eq = 0.0;
        } else {
          xi_eq = max_extent;
        }
        xi_eq = chem_clip(xi_eq, 0.0, max_extent);
      }
      if (!(xi_eq > 1e-30)) continue;
      const double xi_t = chem_clip(xi_eq * (1.0 - exp(-k_eff * dt)), 0.0, xi_eq);

      double cons[CHEM_NR], prod[CHEM_NP], byp[CHEM_NB];
      double total_consumed = 0.0, sum_prod = 0.0, sum_byp = 0.0;
#pragma unroll
      for (int j = 0; j < CHEM_NR; ++j) {
        cons[j] = 0.0;
        if (j < nr) {
          cons[j] = fmin((double)r_k[j] * xi_t, r_mol[j]) * CHEM_PROP(L, 0, chem_ix(ri, 4 + j, L.C));
          total_consumed += cons[j];
        }
      }
#pragma unroll
      for (int j = 0; j < CHEM_NP; ++j) {
        prod[j] = 0.0;
        if (j < np) {
          prod[j] = (double)p_k[j] * xi_t * CHEM_PROP(L, 0, chem_ix(ri, 16 + j, L.C));
          sum_prod += prod[j];
        }
      }
#pragma unroll
      for (int j = 0; j < CHEM_NB; ++j) {
        byp[j] = 0.0;
        if (j < nb) {
          byp[j] = (double)ri[28 + j] * xi_t * CHEM_PROP(L, 0, chem_ix(ri, 24 + j, L.C)) * 0.1;
          sum_byp += byp[j];
        }
      }
      const double total_produced = sum_prod + sum_byp;
      if (total_produced > total_consumed && total_consumed > 1e-12) {
        const double scale = total_consumed / total_produced;
        sum_prod = 0.0;
#pragma unroll
        for (int j = 0; j < CHEM_NP; ++j)
          if (j < np) { prod[j] = prod[j] * scale; sum_prod += prod[j]; }
#pragma unroll
        for (int j = 0; j < CHEM_NB; ++j)
          if (j < nb) byp[j] = byp[j] * scale;
      }
      if (total_consumed + sum_prod < 1e-12) continue;      // :744-746
      progress = true;
      step_heat += xi_t * (-rf[1]) * 1000.0;
      fired[r * CHEM_LANES] += 1;
#pragma unroll
      for (int j = 0; j < CHEM_NR; ++j)
        if (j < nr) {
          const int c = chem_ix(ri, 4 + j, L.C);
          const double actual = fmin(cons[j], CHEM_POOL(L, c));
          if (actual > 1e-12) {
            CHEM_POOL(L, c) -= actual;
            CHEM_ACCUM(0, c) += actual;
          }
        }
#pragma unroll
      for (int j = 0; j < CHEM_NP + CHEM_NB; ++j) {
        const bool is_p = j < CHEM_NP;
        const int jj = is_p ? j : j - CHEM_NP;
        if (jj < (is_p ? np : nb)) {
          const int c = is_p ? chem_ix(ri, 16 + jj, L.C) : chem_ix(ri, 24 + jj, L.C);
          const double g = is_p ? prod[jj] : byp[jj];
          if (g > 1e-12) {
            CHEM_POOL(L, c) += g;
            if (!((member >> c) & 1ull)) {      // a new key of the pool dict
              member |= 1ull << c;
              L.order[L.n_order * CHEM_LANES] = (uint8_t)c;
              ++L.n_order;
            }
            CHEM_ACCUM(is_p ? 1 : 2, c) += g;
          }
        }
      }
    }

    // _update_vessel_state :431-499
    {
      const double old_T = T;
      if (mode == 0) {
        if (max_heat_W > 0.0 && dt > 0.0) {
          const double heat_rate_W = fabs(step_heat) / dt;
          if (heat_rate_W > max_heat_W) {
            const double excess_J = (heat_rate_W - max_heat_W) * dt;
            const double excess_heat = step_heat > 0.0 ? excess_J : -excess_J;
            const double Cp = chem_heat_capacity(L);
            const double phase_heat = chem_phase_heat(L, old_T, old_T + excess_heat / Cp);
            T += (excess_heat - phase_heat) / Cp;
          }
        }
      } else if (mode == 1) {
        const double Cp = chem_heat_capacity(L);
        const double phase_heat = chem_phase_heat(L, old_T, old_T + step_heat / Cp);
        T += (step_heat - phase_heat) / Cp;
      } else if (mode == 2) {
        const double Cp = chem_heat_capacity(L);
        const double net_heat = step_heat - htc * Cp * (T - 25.0) * dt;
        const double phase_heat = chem_phase_heat(L, old_T, old_T + net_heat / Cp);
        T += (net_heat - phase_heat) / Cp;
      } else {
        const double Cp = chem_heat_capacity(L);
        const double total_dT = rate * dt + step_heat / Cp;
        const double phase_heat = chem_phase_heat(L, old_T, old_T + total_dT);
        T += (step_heat + rate * dt * Cp - phase_heat) / Cp;
      }
      T = chem_clip(T, -273.0, 5000.0);
      L.T = T;
      if (sealed) {
        const double gas = chem_gas_moles(L);      // at the new temperature, the old pressure
        const double T_K_now = T + 273.15, T_K_init = T_init + 273.15;
        if (initial_gas_moles > 1e-9) P = P_init * (gas / initial_gas_moles) * (T_K_now / T_K_init);
        else if (gas > 1e-9) P = gas * 8.314 * T_K_now / (volume * 0.001) / 101325.0;
        P = chem_clip(P, 0.001, 1000.0);
        L.logP = log(fmax(0.01, P));
      }
    }
    if (T > max_T || T < min_T) failure = 3;      // :772-806: the batch is destroyed, this step's totals are not counted
    else if (P > max_P) failure = 4;
    if (failure) { failure_step = step; break; }

    if (!sealed) {      // _apply_gas_loss :614-636
      for (int i = 0; i < L.n_order; ++i) {
        const int c = L.order[i * CHEM_LANES];
        const double g = CHEM_POOL(L, c);
        if (g < 1e-9) continue;
        if (chem_state(L, c) == 2) {
          const double escaped = g * (1.0 - retention);
          if (escaped > 1e-12) {
            CHEM_POOL(L, c) = g - escaped;
            CHEM_ACCUM(6, c) += escaped;
          }
        }
      }
    }
    if (!progress) {
      if (++converged_steps >= 3) break;
    } else {
      converged_steps = 0;
    }
    const bool sampled = step < 5 || step % stride == 0;      // :826-843
    const bool log_it = progress && sampled && O.log_step != nullptr && log_count < XV_CHEM_LOG_MAX;
    if (progress) {      // the step's sums join the totals (:819-824) and are cleared for the next step
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double v = CHEM_ACCUM(a, c);
          if (a < 2 && log_it)
            (a == 0 ? O.log_consumed : O.log_produced)[((size_t)e * XV_CHEM_LOG_MAX + log_count) * cs + c] = v;
          if (v != 0.0) {
            CHEM_ACCUM(3 + a, c) += v;
            CHEM_ACCUM(a, c) = 0.0;
          }
        }
      }
    }
    if (sampled && O.hist_step != nullptr && hist_count < XV_CHEM_HISTORY_MAX) {
      const size_t k = (size_t)e * XV_CHEM_HISTORY_MAX + hist_count;
      O.hist_step[k] = step;
      O.hist_T[k] = T;
      O.hist_P[k] = P;
      ++hist_count;
    }
    if (log_it) {
      const size_t k = (size_t)e * XV_CHEM_LOG_MAX + log_count;
      O.log_step[k] = step;
      O.log_active[k] = n_app;
      O.log_T[k] = T;
      O.log_P[k] = P;
      ++log_count;
    }
  }
  X.T = T; X.P = P;
  X.num_steps = num_steps; X.steps_run = steps_run; X.failure = failure; X.failure_step = failure_step;
  X.converged_steps = converged_steps; X.hist_count = hist_count; X.log_count = log_count;
  *errp |= err;
}

// static: chemverse_optimal.hip includes this file, and the kernel is no template
static __global__ __launch_bounds__(CHEM_LANES) void chem_simulate_kernel(ChemWorlds W, ChemExp X, ChemOut O,
                                                                          double* __restrict__ ws_acc,
                                                                          int32_t* __restrict__ ws_fired, uint32_t* err_word) {
  extern __shared__ double chem_smem[];
  const int lane = threadIdx.x;
  const int cs = W.c_stride, rs = W.r_stride;
  double* s_pool = chem_smem;                                   // [cs][64]
  double* s_chem = chem_smem + (size_t)cs * CHEM_LANES;         // [8][cs]
  uint8_t* s_order = reinterpret_cast<uint8_t*>(s_chem + CHEM_F * cs);      // [cs][64]
  const int exp0 = blockIdx.x * CHEM_LANES;
  const int e = exp0 + lane;
  uint32_t err = 0u;

  // the workgroup's world: that of its first experiment
  int wb = X.exp_world[exp0];
  if ((unsigned)wb >= (unsigned)W.n_world) { wb = 0; if (lane == 0) err |= XV_DEVERR_ACTION_RANGE; }
  const ChemWorldAt A = chem_stage_world(W, wb, lane, s_chem, &err);
  const int C = A.C, R = A.R;

  bool active = e < X.n_exp;
  if (active) {
    const int w = X.exp_world[e];
    if (w < 0) active = false;      // a padding lane
    else if (w != wb) { active = false; err |= XV_DEVERR_ACTION_RANGE; }      // the caller groups experiments by world
  }
  if (!active) {
    if (err) atomicOr(err_word, err);
    return;      // no barrier follows
  }

  ChemLane L;
  L.pool = s_pool + lane;
  L.order = s_order + lane;
  L.chem = s_chem;
  L.cs = cs;
  L.C = C;
  double* acc = ws_acc + (size_t)blockIdx.x * CHEM_ACC * cs * CHEM_LANES + lane;      // array a, chemical c: acc[(a * cs + c) * 64]
  int32_t* fired = ws_fired + (size_t)blockIdx.x * rs * CHEM_LANES + lane;
  uint64_t member;
  chem_lane_clear(L, &member, acc, fired, R);

  int n_init = X.n_initial[e];
  if (n_init < 0 || n_init > cs) { err |= XV_DEVERR_ACTION_RANGE; n_init = n_init < 0 ? 0 : cs; }
  for (int i = 0; i < n_init; ++i) {      // :668-671
    const int c = X.order[(size_t)e * cs + i];
    if ((unsigned)c >= (unsigned)C) { err |= XV_DEVERR_ACTION_RANGE; continue; }
    if ((member >> c) & 1ull) continue;
    const double g = X.amounts[(size_t)e * cs + c];
    if (!isfinite(g)) { err |= XV_DEVERR_NONFINITE; continue; }
    chem_lane_charge(L, &member, c, g);
  }
  ChemRun run;
  run.T = X.T[e]; run.P = X.P[e]; run.duration = X.duration[e]; run.rate = X.heating_rate[e]; run.volume = X.volume[e];
  run.eq = X.equipment[e];
  chem_lane_run(W, A, L, member, acc, fired, X.step_seconds, run, O, e, &err);
  const double T = run.T, P = run.P;
  const int num_steps = run.num_steps, steps_run = run.steps_run, failure = run.failure, failure_step = run.failure_step,
            converged_steps = run.converged_steps, hist_count = run.hist_count, log_count = run.log_count;

  // results
  const bool destroyed = failure != 0;
  for (int c = 0; c < cs; ++c) {
    const size_t k = (size_t)e * cs + c;
    const bool in = c < C;
    const double g = in ? CHEM_POOL(L, c) : 0.0;
    if (O.final_pool) O.final_pool[k] = (!destroyed && g > 1e-9) ? g : 0.0;
    if (O.consumed) O.consumed[k] = (in && failure != 1 && failure != 2) ? CHEM_ACCUM(3, c) : 0.0;
    if (O.produced) O.produced[k] = (in && !destroyed) ? CHEM_ACCUM(4, c) : 0.0;
    if (O.byproduct) O.byproduct[k] = (in && !destroyed) ? CHEM_ACCUM(5, c) : 0.0;
    if (O.gas_lost) O.gas_lost[k] = (in && !destroyed) ? CHEM_ACCUM(6, c) : 0.0;
  }
  if (O.fired)
    for (int r = 0; r < rs; ++r) O.fired[(size_t)e * rs + r] = r < R ? fired[r * CHEM_LANES] : 0;
  if (O.num_steps) O.num_steps[e] = num_steps;
  if (O.steps_run) O.steps_run[e] = steps_run;
  if (O.converged) O.converged[e] = (uint8_t)(!destroyed && converged_steps >= 3);
  if (O.failure) O.failure[e] = (uint8_t)failure;
  if (O.failure_step) O.failure_step[e] = failure_step;
  if (O.final_T) O.final_T[e] = T;
  if (O.final_P) O.final_P[e] = P;
  if (O.hist_step) {
    for (int i = hist_count; i < XV_CHEM_HISTORY_MAX; ++i) {
      const size_t k = (size_t)e * XV_CHEM_HISTORY_MAX + i;
      O.hist_step[k] = 0;
      O.hist_T[k] = 0.0;
      O.hist_P[k] = 0.0;
    }
    O.hist_count[e] = hist_count;
  }
  if (O.log_step) {
    for (int i = log_count; i < XV_CHEM_LOG_MAX; ++i) {
      const size_t k = (size_t)e * XV_CHEM_LOG_MAX + i;
      O.log_step[k] = 0;
      O.log_active[k] = 0;
      O.log_T[k] = 0.0;
      O.log_P[k] = 0.0;
      for (int c = 0; c < cs; ++c) {
        O.log_consumed[k * cs + c] = 0.0;
        O.log_produced[k * cs + c] = 0.0;
      }
    }
    for (int i = 0; i < log_count; ++i)      // the columns beyond this world's chemicals
      for (int c = C; c < cs; ++c) {
        O.log_consumed[((size_t)e * XV_CHEM_LOG_MAX + i) * cs + c] = 0.0;
        O.log_produced[((size_t)e * XV_CHEM_LOG_MAX + i) * cs + c] = 0.0;
      }
    O.log_count[e] = log_count;
  }
  if (err) atomicOr(err_word, err);
}

struct xv_chem {
  xv_engine* eng;
  int capacity;
  ChemWorlds w;
  bool worlds_set;
  int blocks;          // workgroups the workspace serves
  double* ws_acc;      // [blocks][7][c_stride][64]
  int32_t* ws_fired;   // [blocks][r_stride][64]
  double* ws_opt;      // the cost oracle's (chemverse_optimal.hip), made by its first call: the virtual pool
                       // [blocks][c_stride][64], then lo, hi, best [blocks * 64] each
  uint32_t* ws_opt_bits;      // [blocks * 64][2]: the decision bits, found
};

#ifndef XV_KERNELS_ONLY      // chemverse_optimal.hip includes this file for its kernels and handle type only
#include <new>

extern "C" int xv_chem_create(xv_engine* e, int n_exp_capacity, xv_chem** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(e != nullptr && n_exp_capacity >= 1);
  if (n_exp_capacity > XV_CHEM_EXP_MAX) {
    xv_set_error("xv_chem_create: n_exp_capacity = %d is beyond the supported XV_CHEM_EXP_MAX = %d", n_exp_capacity,
                 XV_CHEM_EXP_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  xv_chem* h = new (std::nothrow) xv_chem();
  if (!h) {
    xv_set_error("xv_chem_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  h->eng = e;
  h->capacity = n_exp_capacity;
  h->w = ChemWorlds();
  h->worlds_set = false;
  h->blocks = 0;
  h->ws_acc = nullptr;
  h->ws_fired = nullptr;
  h->ws_opt = nullptr;
  h->ws_opt_bits = nullptr;
  *out = h;
  return XV_OK;
}

static void chem_free_workspace(xv_chem* h) {
  if (h->ws_acc) (void)hipFree(h->ws_acc);
  if (h->ws_fired) (void)hipFree(h->ws_fired);
  if (h->ws_opt) (void)hipFree(h->ws_opt);
  if (h->ws_opt_bits) (void)hipFree(h->ws_opt_bits);
  h->ws_acc = nullptr;
  h->ws_fired = nullptr;
  h->ws_opt = nullptr;
  h->ws_opt_bits = nullptr;
  h->blocks = 0;
}

extern "C" int xv_chem_destroy(xv_chem* h) {
  if (!h) return XV_OK;
  (void)hipSetDevice(h->eng->device);
  (void)hipStreamSynchronize(h->eng->stream);
  chem_free_workspace(h);
  delete h;
  return XV_OK;
}

extern "C" int xv_chem_set_worlds(xv_chem* h, int n_world, int c_stride, int r_stride, const int32_t* world_off,
                                  const double* chem_f, const uint8_t* sol_present, const double* sol_value,
                                  const int32_t* rxn_i, const double* rxn_f, const int64_t* rxn_solv, const int32_t* eq_i,
                                  const double* eq_f) {
  XV_CHECK_ARG(h != nullptr && n_world >= 1 && c_stride >= 1 && r_stride >= 1);
  XV_CHECK_ARG(world_off && chem_f && sol_present && sol_value && rxn_i && rxn_f && rxn_solv && eq_i && eq_f);
  if (c_stride > XV_CHEM_C_MAX) {
    xv_set_error("xv_chem_set_worlds: c_stride = %d chemicals is beyond the supported XV_CHEM_C_MAX = %d", c_stride,
                 XV_CHEM_C_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  if (r_stride > XV_CHEM_R_MAX) {
    xv_set_error("xv_chem_set_worlds: r_stride = %d reactions is beyond the supported XV_CHEM_R_MAX = %d", r_stride,
                 XV_CHEM_R_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  if (n_world > XV_CHEM_WORLDS_MAX) {
    xv_set_error("xv_chem_set_worlds: n_world = %d is beyond the supported XV_CHEM_WORLDS_MAX = %d", n_world,
                 XV_CHEM_WORLDS_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  XV_HIP(hipStreamSynchronize(e->stream));      // a running launch reads the tables and the workspace let go below
  chem_free_workspace(h);
  h->worlds_set = false;
  const int blocks = xv_div_up(h->capacity, CHEM_LANES) + n_world;      // every world may end in a partly filled workgroup
  XV_HIP(hipMalloc(&h->ws_acc, (size_t)blocks * CHEM_ACC * c_stride * CHEM_LANES * sizeof(double)));
  XV_HIP(hipMalloc(&h->ws_fired, (size_t)blocks * r_stride * CHEM_LANES * sizeof(int32_t)));
  h->blocks = blocks;
  ChemWorlds& w = h->w;
  w.n_world = n_world; w.c_stride = c_stride; w.r_stride = r_stride;
  w.world_off = world_off; w.chem_f = chem_f; w.sol_present = sol_present; w.sol_value = sol_value;
  w.rxn_i = rxn_i; w.rxn_f = rxn_f; w.rxn_solv = rxn_solv; w.eq_i = eq_i; w.eq_f = eq_f;
  h->worlds_set = true;
  return XV_OK;
}

extern "C" int xv_chem_simulate(xv_chem* h, int n_exp, const int32_t* exp_world, const double* amounts, const int32_t* order,
                                const int32_t* n_initial, const double* temperature_C, const double* pressure_atm,
                                const double* duration_s, const int32_t* equipment, const double* heating_rate_C_per_s,
                                const double* vessel_volume_L, double step_seconds, const xv_chem_out* out) {
  XV_CHECK_ARG(h != nullptr && n_exp >= 1 && out != nullptr);
  XV_CHECK_ARG(exp_world && amounts && order && n_initial && temperature_C && pressure_atm && duration_s && equipment &&
               heating_rate_C_per_s && vessel_volume_L);
  XV_CHECK_ARG(step_seconds > 0.0 && step_seconds <= 1.7e308);
  if (!h->worlds_set) {
    xv_set_error("xv_chem_simulate: no worlds set (xv_chem_set_worlds)");
    return XV_ERR_INVALID;
  }
  const int blocks = xv_div_up(n_exp, CHEM_LANES);
  if (blocks > h->blocks) {
    xv_set_error("xv_chem_simulate: n_exp = %d needs %d workgroups, the handle (capacity %d, %d worlds) serves %d", n_exp,
                 blocks, h->capacity, h->w.n_world, h->blocks);
    return XV_ERR_INVALID;
  }
  const int hist = (out->hist_step != nullptr) + (out->hist_T != nullptr) + (out->hist_P != nullptr) + (out->hist_count != nullptr);
  const int log = (out->log_step != nullptr) + (out->log_active != nullptr) + (out->log_T != nullptr) +
                  (out->log_P != nullptr) + (out->log_consumed != nullptr) + (out->log_produced != nullptr) +
                  (out->log_count != nullptr);
  if ((hist != 0 && hist != 4) || (log != 0 && log != 7)) {
    xv_set_error("xv_chem_simulate: the temperature history is its four arrays or none, the reaction log its seven or none");
    return XV_ERR_INVALID;
  }
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  ChemExp x;
  x.exp_world = exp_world; x.amounts = amounts; x.order = order; x.n_initial = n_initial;
  x.T = temperature_C; x.P = pressure_atm; x.duration = duration_s; x.equipment = equipment;
  x.heating_rate = heating_rate_C_per_s; x.volume = vessel_volume_L; x.step_seconds = step_seconds; x.n_exp = n_exp;
  ChemOut o;
  o.final_pool = out->final_pool; o.consumed = out->consumed; o.produced = out->produced; o.byproduct = out->byproduct;
  o.gas_lost = out->gas_lost; o.fired = out->fired; o.num_steps = out->num_steps; o.steps_run = out->steps_run;
  o.converged = out->converged; o.failure = out->failure; o.failure_step = out->failure_step; o.final_T = out->final_T;
  o.final_P = out->final_P; o.hist_step = out->hist_step; o.hist_T = out->hist_T; o.hist_P = out->hist_P;
  o.hist_count = out->hist_count; o.log_step = out->log_step; o.log_active = out->log_active; o.log_T = out->log_T;
  o.log_P = out->log_P; o.log_consumed = out->log_consumed; o.log_produced = out->log_produced; o.log_count = out->log_count;
  const size_t lds = (size_t)h->w.c_stride * (CHEM_LANES * sizeof(double) + CHEM_F * sizeof(double) + CHEM_LANES);
  hipLaunchKernelGGL(chem_simulate_kernel, dim3((unsigned)blocks), dim3(CHEM_LANES), lds, e->stream, h->w, x, o, h->ws_acc,
                     h->ws_fired, e->d_err);
  XV_LAUNCH_CHECK();
  return XV_OK;
}
#endif
