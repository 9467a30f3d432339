// dp_lm_terms_dev.h -- device helpers of dp_lm_terms.hip alone (dp_lm_body.h with DP_LM_TERMS 1); included after dp_lm_dev.h.
#pragma once

namespace {

using dpcons::T_TYPE, dpcons::T_JA, dpcons::T_JB, dpcons::T_FLAGS, dpcons::T_W, dpcons::T_PT, dpcons::T_DIR, dpcons::T_AXA, dpcons::T_AXB, dpcons::T_P0,
    dpcons::T_P1, dpcons::T_ROW; // the staged term's words (dp_cons.h)

// Column cn of d P_jj / dz (dP[3]) and of d G_jj / dz (dG[9]), unscaled, for any joint jj: what the tracker loop of dp_lm_body.h forms for a
// tracked joint, in its order -- the bones of jj's path, each through its parent's quaternion, and the root's part (dR0, dwd: d R_0 and
// d world_disp of the same column).  TB: the tangents d(decoder output)/dz; QN, RN, RB, VB: the forward pass's unit quaternions, 1 / |q_j|,
// R_j and v_j; off: the bone offsets [22][3].  What the caller does not read is not computed (the function is inlined).
DEV void joint_tangent(int jj, int cn, const int* par, const float* off, const float* TB, const float* QN, const float* RN, const float* RB, const float* VB,
                       const float* R0, const float* dR0, const float* dwd, float* dP, float* dG)
{
    float dv[3] = {0.f, 0.f, 0.f}; // d v_jj
    int c = jj;
    for (int s = 0; s < NJ && c != 0; ++s) {
        const int p = par[c];
        if (p != 0) {
            float dq[4], dqn[4], dRp[9], t[3];
#pragma unroll
            for (int e = 0; e < 4; ++e) dq[e] = TB[(4 * p + e) * ST + cn];
            unit_jvp(QN + 4 * p, RN[p], dq, dqn);
            rotmat_jvp(QN + 4 * p, dqn, dRp);
            mv(dRp, off + 3 * c, t);
            dv[0] += t[0]; dv[1] += t[1]; dv[2] += t[2];
        }
        c = p;
    }
    float t0[3], t1[3];
    mv(dR0, VB + 4 * jj, t0);
    mv(R0, dv, t1);
#pragma unroll
    for (int e = 0; e < 3; ++e) dP[e] = (dwd[e] + t0[e]) + t1[e];
    if (jj == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) dG[k] = dR0[k];
    } else {
        float dq[4], dqn[4], dRj[9];
#pragma unroll
        for (int e = 0; e < 4; ++e) dq[e] = TB[(4 * jj + e) * ST + cn];
        unit_jvp(QN + 4 * jj, RN[jj], dq, dqn);
        rotmat_jvp(QN + 4 * jj, dqn, dRj);
        const float* Rj = RB + 9 * jj;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int e = 0; e < 3; ++e)
                dG[3 * r + e] = (dR0[3 * r] * Rj[e] + dR0[3 * r + 1] * Rj[3 + e] + dR0[3 * r + 2] * Rj[6 + e]) +
                                (R0[3 * r] * dRj[e] + R0[3 * r + 1] * dRj[3 + e] + R0[3 * r + 2] * dRj[6 + e]);
    }
}

DEV float t_sqrt(float x) { return sqrtf(x); }
DEV double t_sqrt(double x) { return sqrt(x); }
DEV float t_fma(float a, float b, float c) { return fmaf(a, b, c); }
DEV double t_fma(double a, double b, double c) { return fma(a, b, c); }

// h(v): the up component set to 0, without indexing registers at run time
template <class T>
DEV void flatten(T* v, int up)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = c == up ? (T)0 : v[c];
}

// ws * T of one term (include/dragposer_terms.h) in T's arithmetic -- dp_cons_body.h's formulas.  tb: the staged term; row: the frame's row
// (vector, s_f); ws = weight * s_f; P: the joints' positions, row stride ps; G: their rotations [22][9]; gp: global_pos
template <class T>
DEV T term_value(const float* tb, const float* row, float ws, const T* P, int ps, const T* G, const float* gp, int up)
{
    const int* ti = (const int*)tb;
    const int type = ti[T_TYPE], ja = ti[T_JA], jb = ti[T_JB], fl = ti[T_FLAGS];
    const bool drop = (fl & DP_TERM_DROP_UP) != 0;
    T val = (T)0;
    if (type == DP_TERM_PLANE) { // d = dir . (g + P_a - point)
        T dd = (T)0;
#pragma unroll
        for (int c = 0; c < 3; ++c) dd = t_fma((T)tb[T_DIR + c], ((T)gp[c] + P[ps * ja + c]) - (T)row[c], dd);
        T g = dd;
        if (fl & DP_TERM_ONE_SIDED) g = dd < (T)0 ? dd : (T)0; // -relu(-d)
        val = (T)ws * (g * g);
    } else if (type == DP_TERM_DISTANCE) { // q = |h(P_a - P_b)|^2 or |h(g + P_a - point)|^2
        T u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = jb >= 0 ? P[ps * ja + c] - P[ps * (jb < 0 ? 0 : jb) + c] : ((T)gp[c] + P[ps * ja + c]) - (T)row[c];
        if (drop) flatten(u, up);
        const T q = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
        const T xh = q - (T)tb[T_P1], xl = (T)tb[T_P0] - q; // (p0, p1 staged as lo^2, hi^2)
        val = (T)ws * ((xh > (T)0 ? xh : (T)0) + (xl > (T)0 ? xl : (T)0));
    } else { // DP_TERM_ALIGN: u = h(G_a axis_a), v = h(G_b axis_b) or h(dir)
        T av[3], bv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            av[r] = G[9 * ja + 3 * r] * (T)tb[T_AXA] + G[9 * ja + 3 * r + 1] * (T)tb[T_AXA + 1] + G[9 * ja + 3 * r + 2] * (T)tb[T_AXA + 2];
        if (drop) flatten(av, up);
        const T na = t_sqrt(av[0] * av[0] + av[1] * av[1] + av[2] * av[2]);
        if (na > (T)tb[T_P0]) {
            const int jq = jb < 0 ? 0 : jb;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                bv[r] = jb >= 0 ? G[9 * jq + 3 * r] * (T)tb[T_AXB] + G[9 * jq + 3 * r + 1] * (T)tb[T_AXB + 1] + G[9 * jq + 3 * r + 2] * (T)tb[T_AXB + 2]
                                : (T)row[r];
            if (drop) flatten(bv, up);
            const T nb = t_sqrt(bv[0] * bv[0] + bv[1] * bv[1] + bv[2] * bv[2]);
            const T cs = (av[0] / na) * (bv[0] / nb) + (av[1] / na) * (bv[1] / nb) + (av[2] / na) * (bv[2] / nb);
            const T sc = cs + (T)tb[T_P1];
            if (sc < (T)1) {
                const T w1 = (T)1 - sc;
                val = (T)ws * (w1 * w1);
            }
        }
    }
    return val;
}

// The rows of [J | r] of one term at the kept latent (include/dragposer_lm_terms.h, "The algorithm"), for this lane's column: r3[0..2], zero
// where the term has no row.  cn < 24: column cn of the rows (the tangents of the term's joints come from joint_tangent); cn == 24: the
// residuals.  The active set is taken here, with strict inequalities.  PB [22][4] and GB [22][9]: the kept latent's P_j and G_j.
DEV void term_rows(const float* tb, const float* row, int cn, const float* PB, const float* GB, const float* gp, int up, const int* par, const float* off,
                   const float* TB, const float* QN, const float* RN, const float* RB, const float* VB, const float* R0, const float* dR0, const float* dwd,
                   float* r3)
{
    const int* ti = (const int*)tb;
    const int type = ti[T_TYPE], ja = ti[T_JA], jb = ti[T_JB], fl = ti[T_FLAGS];
    const bool drop = (fl & DP_TERM_DROP_UP) != 0, col = cn < LAT;
    const float sc = sqrtf(tb[T_W] * row[3]); // sqrt(c_k)
    r3[0] = r3[1] = r3[2] = 0.f;
    // what the term is at z: kind 0 no row, 1 PLANE, 2 DISTANCE above hi, 3 DISTANCE below lo, 4 ALIGN; u, w and the ALIGN's da, db
    int kind = 0;
    float u[3] = {0.f, 0.f, 0.f}, w = 0.f, da[3] = {0.f, 0.f, 0.f}, db[3] = {0.f, 0.f, 0.f};
    if (type == DP_TERM_PLANE) {
        float dd = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) dd = fmaf(tb[T_DIR + c], (gp[c] + PB[4 * ja + c]) - row[c], dd);
        w = dd;
        kind = (!(fl & DP_TERM_ONE_SIDED) || dd < 0.f) ? 1 : 0;
    } else if (type == DP_TERM_DISTANCE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = jb >= 0 ? PB[4 * ja + c] - PB[4 * (jb < 0 ? 0 : jb) + c] : (gp[c] + PB[4 * ja + c]) - row[c];
        if (drop) flatten(u, up);
        const float q = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
        if (q > tb[T_P1]) kind = 2;
        else if (q < tb[T_P0]) {
            kind = 3;
            w = sqrtf(tb[T_P0] - q);
        }
    } else {
        float av[3], bv[3];
        mv(GB + 9 * ja, tb + T_AXA, av);
        if (drop) flatten(av, up);
        const float na = sqrtf(av[0] * av[0] + av[1] * av[1] + av[2] * av[2]);
        if (na > tb[T_P0]) {
            if (jb >= 0) mv(GB + 9 * jb, tb + T_AXB, bv);
            else
#pragma unroll
                for (int c = 0; c < 3; ++c) bv[c] = row[c];
            if (drop) flatten(bv, up);
            const float nb = sqrtf(bv[0] * bv[0] + bv[1] * bv[1] + bv[2] * bv[2]);
            float ah[3], bh[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { ah[c] = av[c] / na; bh[c] = bv[c] / nb; }
            const float cs = ah[0] * bh[0] + ah[1] * bh[1] + ah[2] * bh[2];
            const float s = cs + tb[T_P1];
            if (s < 1.f) {
                kind = 4;
                w = 1.f - s;
#pragma unroll
                for (int c = 0; c < 3; ++c) { da[c] = (bh[c] - ah[c] * cs) / na; db[c] = (ah[c] - bh[c] * cs) / nb; } // d c / d u, d c / d v
                if (drop) { flatten(da, up); flatten(db, up); }
            }
        }
    }
    if (kind == 0) return;
    if (!col) { // the residuals
        if (kind == 2) {
#pragma unroll
            for (int e = 0; e < 3; ++e) r3[e] = sc * u[e];
        } else r3[0] = sc * w; // sqrt(c) d, sqrt(c (lo^2 - q)), sqrt(c) (1 - c)
        return;
    }
    float dPa[3], dGa[9], dPb[3] = {0.f, 0.f, 0.f}, dGb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) dGb[k] = 0.f;
    joint_tangent(ja, cn, par, off, TB, QN, RN, RB, VB, R0, dR0, dwd, dPa, dGa);
    if (jb >= 0) joint_tangent(jb, cn, par, off, TB, QN, RN, RB, VB, R0, dR0, dwd, dPb, dGb);
    if (kind == 1) r3[0] = sc * (tb[T_DIR] * dPa[0] + tb[T_DIR + 1] * dPa[1] + tb[T_DIR + 2] * dPa[2]);
    else if (kind == 4) {
        float ta[3], tv[3];
        mv(dGa, tb + T_AXA, ta);
        mv(dGb, tb + T_AXB, tv);
        r3[0] = -sc * ((da[0] * ta[0] + da[1] * ta[1] + da[2] * ta[2]) + (db[0] * tv[0] + db[1] * tv[1] + db[2] * tv[2]));
    } else {
        float du[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) du[e] = dPa[e] - dPb[e];
        if (drop) flatten(du, up);
        if (kind == 2) {
#pragma unroll
            for (int e = 0; e < 3; ++e) r3[e] = sc * du[e];
        } else r3[0] = -sc * (u[0] * du[0] + u[1] * du[1] + u[2] * du[2]) / w;
    }
}

} // namespace
