/* mz_wall_stage.inc — body of maze_view's wall loop for one screen column d_h (ray_caster_utils.py:247-318 with DDA_2D
 * :47-115), written once over REAL and included twice by mz_view (xeno_oracle.c):
 *   REAL = float   the typing the reference's source has when its @njit functions run as plain Python under NumPy 2
 *                  (Python floats are weak: float32 table entries keep the DDA and the wall-column geometry in float32)
 *                  — this is what tests/golden/maze_*.npz were generated with and what the device reproduces;
 *   REAL = double  the typing numba gives the same source (float32 op float64 -> float64: DDA_2D and the wall-column
 *                  geometry run in float64).  numba is not installed here, so this variant is unpinned; it exists to
 *                  measure how far the two typings are apart (tests/test_oracle_maze.py). */
    const int i0 = (int)(pos[0] / cs_f), j0 = (int)(pos[1] / cs_f); /* :248-249, outside DDA_2D: float32 / python float */
    /* ---- DDA_2D :47-115 in REAL ---- */
    const float co32 = cos_abs[d_h], so32 = sin_abs[d_h];
    const REAL co = (REAL)co32, so = (REAL)so32, cs_r = (REAL)cell_size, eps_r = (REAL)1.0e-8, vis_r = (REAL)visibility, lf_r = (REAL)l_focal;
    const REAL c_sign = co < 0 ? (REAL)-1 : (REAL)1, s_sign = so < 0 ? (REAL)-1 : (REAL)1;
    const REAL ddx = RFABS(co) < eps_r ? RFABS(cs_r / eps_r) : RFABS(cs_r / co);
    const REAL ddy = RFABS(so) < eps_r ? RFABS(cs_r / eps_r) : RFABS(cs_r / so);
    const REAL d_x = co > 0 ? ((REAL)((i0 + 1) * cell_size) - (REAL)pos[0]) : ((REAL)(i0 * cell_size) - (REAL)pos[0]);
    const REAL d_y = so > 0 ? ((REAL)((j0 + 1) * cell_size) - (REAL)pos[1]) : ((REAL)(j0 * cell_size) - (REAL)pos[1]);
    REAL sdx = RFABS(co) < eps_r ? c_sign * (d_x / eps_r) : d_x / co;
    REAL sdy = RFABS(so) < eps_r ? s_sign * (d_y / eps_r) : d_y / so;
    const int di = co > 0 ? 1 : -1, dj = so > 0 ? 1 : -1;
    int hi = i0, hj = j0, hit_side = 0, n_tr = 0;
    REAL hit_dist = 0;
    REAL tr_dist[64];
    int tr_id[64];
    while (hit_dist < vis_r) {
      if (sdx < sdy) {
        hi += di; sdy -= sdx; hit_dist += sdx;
        if (transp[hi * NG + hj] > -1 && n_tr < 64) { tr_dist[n_tr] = hit_dist; tr_id[n_tr++] = transp[hi * NG + hj]; }
        if (hi < 0 || hi >= n) { if (hj < 0 || hj >= n) { hit_dist = (REAL)1.0e+6; break; } }
        else if (walls[hi * NG + hj] > 0) { hit_side = 0; break; }
        sdx = ddx;
      } else {
        hj += dj; sdx -= sdy; hit_dist += sdy;
        if (transp[hi * NG + hj] > -1 && n_tr < 64) { tr_dist[n_tr] = hit_dist; tr_id[n_tr++] = transp[hi * NG + hj]; }
        if (hi < 0 || hi >= n) { if (hj < 0 || hj >= n) { hit_dist = (REAL)1.0e+6; break; } }
        else if (walls[hi * NG + hj] > 0) { hit_side = 1; break; }
        sdy = ddy;
      }
    }
    /* ---- wall column :258-298 ---- */
    REAL alpha = (REAL)2 * hit_dist / vis_r - (REAL)1;
    if (alpha < 0) alpha = 0;
    if (alpha > 1) alpha = 1;
    const int text_id = texts[hi * NG + hj];
    const REAL hit_pt_x = hit_dist * co + (REAL)pos[0], hit_pt_y = hit_dist * so + (REAL)pos[1];
    REAL local_h;
    float light;
    if (hit_side == 0) { local_h = hit_pt_y / cs_r; local_h -= RFLOOR(local_h); light = fabsf(co32); }
    else { local_h = hit_pt_x / cs_r; local_h -= RFLOOR(local_h); light = fabsf(so32); }
    REAL ratio = hit_dist * (REAL)cos_hp_a[d_h] / lf_r;
    if (RFABS(ratio) < eps_r) ratio = ratio > 0 ? eps_r : -eps_r;
    const REAL top_v = (REAL)(ceil_height - vision_height) / ratio, bot_v = (REAL)vision_height / ratio;
    int v_s = (int)((half_v - (double)top_v) / pixel_size), v_e = (int)((half_v + (double)bot_v) / pixel_size);
    if (v_s < 0) v_s = 0;
    if (v_e > H) v_e = H;
    const float* wt = h->tex_walls + (size_t)text_id * 256 * 256 * 3;
    for (int d_v = v_s; d_v < v_e; ++d_v) {
      const double local_v = (half_v - (d_v + 0.5) * pixel_size) * (double)ratio + vision_height;
      REAL d_i = local_h * (REAL)percell;
      double d_j = local_v / text_size;
      d_i -= RFLOOR(d_i); d_j -= floor(d_j);
      const int ti = (int)((REAL)256 * d_i), tj = (int)(256 * d_j);
      const double eff_ps = eff_distance * pixel_size / l_focal; /* stale eff_distance: quirk (i) */
      double col[3];
      mz_interpolate(wt, (double)ti, (double)tj, eff_ps, tps, tps, col, !typing_f64);
      int32_t* px = rgb + ((size_t)d_h * H + d_v) * 3;
      for (int c = 0; c < 3; ++c) {
        const double blend = (double)(REAL)(alpha * (REAL)1) + (double)((REAL)1 - alpha) * col[c];
        px[c] = mz_clip_int((double)light * blend);
      }
    }
    /* ---- transparent landmark overlays, far to near :301-318 ---- */
    for (int q = n_tr - 1; q >= 0; --q) {
      const REAL hd = tr_dist[q];
      REAL r2 = hd * (REAL)cos_hp_a[d_h] / lf_r;
      if (RFABS(r2) < eps_r) r2 = r2 > 0 ? eps_r : -eps_r;
      const REAL tv = (REAL)(ceil_height - vision_height) / r2, bv = (REAL)vision_height / r2;
      int s2 = (int)((half_v - (double)tv) / pixel_size), e2 = (int)((half_v + (double)bv) / pixel_size);
      if (s2 < 0) s2 = 0;
      if (e2 > H) e2 = H;
      REAL a2 = (REAL)2 * hd / vis_r - (REAL)1;
      if (a2 < 0) a2 = 0;
      if (a2 > 1) a2 = 1;
      for (int d_v = s2; d_v < e2; ++d_v) {
        int32_t* px = rgb + ((size_t)d_h * H + d_v) * 3;
        for (int c = 0; c < 3; ++c) {
          const REAL inner = ((REAL)1 - a2) * (REAL)MZ_LANDMARK_RGB[tr_id[q]][c] + a2 * (REAL)1;
          const REAL tinted = (REAL)0.30 * inner;
          px[c] = mz_clip_int((1.0 - 0.30) * (double)px[c] + (double)tinted);
        }
      }
    }
