// ccp_grid_mgl.hpp — alternating zebra line relaxation for the V-cycle of weighted grid handles
// (CCP_MG_SMOOTHER_LINE, include/ccp_gs.h: ccp_grid_mg_set_smoother), hand-written for gfx950.
//
// What it replaces.  On every level above the tail (k < MgHierarchy::tail) the red-black tile pass k_mg_tile gives way
// to line solves; k_mg_restrict, k_mg_tail, the 1x1 case and the PCG loop are the point mode's, untouched.  Only stored
// operators (kind kMgCoarse: a weighted handle's level 0 and every coarse level) are served, fp64, one channel at a time.
//
// One smoothing sweep is four half passes over a level: the x-lines (rows) of even y, the x-lines of odd y, the y-lines
// (columns) of even x, the y-lines of odd x.  A half pass solves every line of its parity exactly: the cells of the
// line are the unknowns of a tridiagonal system  -w(i-1) z(i-1) + d(i) z(i) - w(i) z(i+1) = b(i) + wN zN + wS zS  (a
// row; a column has wW zW + wE zE on the right), whose right-hand side reads the two neighbouring lines, which belong
// to the other parity and are not written by this pass.  The line's old values are not read at all.  Pre-smoothing
// runs nu sweeps from z = 0 in that order (the very first half pass takes b alone and reads no z); post-smoothing runs
// nu sweeps in the exact reverse order (y odd, y even, x odd, x even), so M stays symmetric.  The prolongation
// z + cs * e_c is fused into the first post half pass: it is formed on the fly for the neighbouring (even) columns the
// pass reads and never stored, because the pass after it overwrites those columns from the odd ones alone.
//
// No pivoting.  d = lambda + the sum of all four weights and the off-diagonals are -w <= 0, so every line system is
// (weakly) diagonally dominant with a positive diagonal, and so are its Schur complements: Thomas elimination, the
// partition below and cyclic reduction all run without pivoting and never meet a zero pivot.  A dead cell (d = 0, a
// fixed pixel: its edges are already cut) becomes the identity row with right-hand side 0, so a line falls apart into
// independent segments there, z = 0 is written on it and nothing divides by a zero diagonal.
//
// The partitioned solve.  A line of n cells is served by L lanes, a power of two chosen from n and the direction
// (mgl_lanes: about kMglChunk cells per lane, at most 256 lanes for a row and at most kMglColumnLanes = 16 for a column),
// lane j owning the contiguous chunk [s, e].  With x_p the last unknown of the chunk before
// and x_e this chunk's last one, every interior cell i in [s, e) is  z(i) = y(i) - v(i) x_p - w(i) x_e:
//   pass 1 (forward over the interior, Thomas): c'(i), y'(i), v'(i) to the work planes;
//   pass 2 (backward): y(i), v(i), w(i) in place of them;
//   the L last unknowns form a tridiagonal interface system (row e with z(e-1) and the next chunk's z(s) substituted),
//   solved across the workgroup by parallel cyclic reduction in LDS, log2 L steps;
//   pass 3: z(i) = y(i) - v(i) x_p - w(i) x_e, and z(e) = x_e.
// A workgroup of 256 threads serves G = 256 / L lines.  Rows: a lane's chunk is contiguous in x, neighbouring lanes own
// neighbouring chunks, so a wave's 64 lanes read 64 places m cells apart in one row (m <= 16 up to W = 4096, 64 at
// 16384): strided, not coalesced.  Columns: the G lanes that share a row segment own G neighbouring columns of the same
// parity, consecutive doubles of one colour plane in every row they march through; the cap of 16 lanes per column keeps
// G >= 16, a run of at least 128 B per row and segment (a wave of 64 lanes covers 64 / G <= 4 such runs, one per
// segment), whatever H is.  A column longer than 256 rows therefore has chunks longer than kMglChunk (4096 rows: 256
// rows per lane), which the work planes allow.  Lanes per half pass of a W x H level: rows ceil(H/2) x L(W), columns
// ceil(W/2) x L(H); at 4096 x 4096 that is 2,048 x 256 lanes = 8,192 waves for a row pass and 2,048 x 16 lanes = 512
// waves for a column pass.
//
// Work planes.  c' / w, y' / y and v' / v of every cell of the level in flight: three planes of the largest line level,
// 3 x (level 0's channel stride) doubles = 24 B per pixel, allocated with the first line V-cycle of a hierarchy and
// freed when the handle goes back to the point smoother.  LDS: 12 x 256 doubles (the interface rows a, b, c, r double
// buffered, the chunks' first y, v, w, the interface solution) = kMglLdsBytes = 24,576 B, all static.  Every launch
// returns at once when st->active is 0.
#pragma once

#include "ccp_grid_mg.hpp"

namespace ccp {

enum MglDir { kMglX = 0, kMglY = 1 };

constexpr int kMglChunk = 16;                                     // cells per lane the lane count aims at
constexpr int kMglColumnLanes = 16;                               // most lanes per column: 256 / 16 = 16 neighbouring columns per row segment
constexpr int kMglLdsBytes = 12 * kBlock * (int)sizeof(double);   // the kernel's static LDS

// lanes per line of n cells: the smallest power of two with at most kMglChunk cells per lane, at most kBlock for a row
// and kMglColumnLanes for a column (longer chunks then)
inline int mgl_lanes(int dir, int n)
{
    const int most = dir == kMglY ? kMglColumnLanes : kBlock;
    int L = 1;
    while (L < most && (long)L * kMglChunk < n) L *= 2;
    return L;
}

// DIR: rows (kMglX) or columns (kMglY) of parity `parity`.  FIRST: z_in is all zero and not read.  ADD: the neighbouring
// lines' values are z_in + cs * e_c on live cells (the prolongation, fused).  z_in and z_out may be the same buffer: the
// pass reads the other parity's lines only.  wy, wv, ww: the work planes (the level's layout).  L: lanes per line.
// grid = ceil(lines of this parity / (kBlock / L)).
template <int DIR, bool FIRST, bool ADD>
__global__ void __launch_bounds__(kBlock)
k_mgl_lines(MgLevel lv, const double *__restrict__ b, const double *z_in, double *z_out, double *__restrict__ wy,
            double *__restrict__ wv, double *__restrict__ ww, MgLevel cv, const double *__restrict__ ec, double cs, int parity, int L,
            const CgState *__restrict__ st)
{
    __shared__ double sa[2][kBlock], sb[2][kBlock], sc[2][kBlock], sr[2][kBlock];
    __shared__ double sfy[kBlock], sfv[kBlock], sfw[kBlock], sx[kBlock];
    static_assert(sizeof(sa) + sizeof(sb) + sizeof(sc) + sizeof(sr) + 4 * sizeof(sx) == kMglLdsBytes, "kMglLdsBytes");
    if (st && !st->active) return;                                   // (uniform)
    const int G = kBlock / L;
    const int lb = DIR == kMglX ? (int)threadIdx.x / L : (int)threadIdx.x % G;
    const int seg = DIR == kMglX ? (int)threadIdx.x % L : (int)threadIdx.x / G;
    const int slot = lb * L + seg;
    const int n = DIR == kMglX ? lv.W : lv.H;                        // cells of a line
    const int across = DIR == kMglX ? lv.H : lv.W;
    const int line = 2 * ((int)blockIdx.x * G + lb) + parity;
    const int m = (n + L - 1) / L;
    const int s = seg * m, e = min(n, s + m) - 1;                    // the lane's chunk [s, e]
    const bool has = line < across && s < n;

    auto at_of = [&](int i) -> long { return DIR == kMglX ? mg_at(lv.pitch, i, line) : mg_at(lv.pitch, line, i); };
    auto along = [&](long at) -> double { return DIR == kMglX ? lv.we[at] : lv.ws[at]; };   // the weight between i and i + 1
    // the value a neighbouring line contributes at (x, y), inside the level
    auto zval = [&](int x, int y) -> double {
        const long a = mg_at(lv.pitch, x, y);
        double z = z_in[a];
        if (ADD && lv.d[a] != 0.0) z = z + cs * ec[mg_at(cv.pitch, x >> 1, y >> 1)];   // (cs * e_c is exact)
        return z;
    };
    // row i of the line's system: diagonal, the weight towards i + 1, the right-hand side; a dead cell is the identity row
    auto row = [&](int i, double &d, double &wn, double &rhs, bool &dead) -> long {
        const long at = at_of(i);
        d = lv.d[at];
        dead = d == 0.0;
        if (dead) {
            d = 1.0;
            wn = 0.0;
            rhs = 0.0;
            return at;
        }
        wn = i + 1 < n ? along(at) : 0.0;
        rhs = b[at];
        if (!FIRST) {
            const int x = DIR == kMglX ? i : line, y = DIR == kMglX ? line : i;
            if (DIR == kMglX) {
                if (y > 0) rhs += lv.ws[mg_at(lv.pitch, x, y - 1)] * zval(x, y - 1);
                if (y + 1 < lv.H) rhs += lv.ws[at] * zval(x, y + 1);
            } else {
                if (x > 0) rhs += lv.we[mg_at(lv.pitch, x - 1, y)] * zval(x - 1, y);
                if (x + 1 < lv.W) rhs += lv.we[at] * zval(x + 1, y);
            }
        }
        return at;
    };

    // the last interior cell's y, v, w (no interior: z(e-1) is x_p itself) and the first one's (z(s) is x_e itself)
    double yl = 0.0, vl = -1.0, wl = 0.0, yf = 0.0, vf = 0.0, wf = -1.0;
    double A = 0.0, B = 1.0, C = 0.0, R = 0.0;                       // the lane's interface row (no chunk: the identity)
    if (has) {
        double wprev = s > 0 ? along(at_of(s - 1)) : 0.0;            // the weight between i - 1 and i
        double cp = 0.0, y = 0.0, v = 0.0;
        for (int i = s; i < e; ++i) {                                // pass 1
            double d, wn, rhs;
            bool dead;
            const long at = row(i, d, wn, rhs, dead);
            const double lo = dead ? 0.0 : -wprev;
            if (i == s) {
                y = rhs / d;
                v = lo / d;
                cp = -wn / d;
            } else {
                const double den = d - lo * cp;
                y = (rhs - lo * y) / den;
                v = (0.0 - lo * v) / den;
                cp = -wn / den;
            }
            wy[at] = y;
            wv[at] = v;
            ww[at] = cp;
            wprev = wn;
        }
        double de, we_, rhse;
        bool deade;
        row(e, de, we_, rhse, deade);
        const double loe = deade ? 0.0 : -wprev;
        if (e > s) {
            yl = y;
            vl = v;
            wl = cp;
            double w = cp;
            for (int i = e - 2; i >= s; --i) {                       // pass 2
                const long at = at_of(i);
                const double c = ww[at];
                y = wy[at] - c * y;
                v = wv[at] - c * v;
                w = 0.0 - c * w;
                wy[at] = y;
                wv[at] = v;
                ww[at] = w;
            }
            yf = y;
            vf = v;
            wf = w;
        }
        sfy[slot] = yf;
        sfv[slot] = vf;
        sfw[slot] = wf;
        A = loe;                                                     // (completed below, once the next chunk's y, v, w are known)
        B = de;
        C = -we_;
        R = rhse;
    } else {
        sfy[slot] = 0.0;
        sfv[slot] = 0.0;
        sfw[slot] = 0.0;
    }
    __syncthreads();
    {
        const bool next = seg + 1 < L;
        const double yn = next ? sfy[slot + 1] : 0.0, vn = next ? sfv[slot + 1] : 0.0, wn = next ? sfw[slot + 1] : 0.0;
        const double lo = A, up = C;                                 // row e: lo z(e-1) + B z(e) + up z(e+1) = R
        A = -(lo * vl);
        B = (B - lo * wl) - up * vn;
        C = -(up * wn);
        R = (R - lo * yl) - up * yn;
    }
    int cur = 0;
    sa[0][slot] = A;
    sb[0][slot] = B;
    sc[0][slot] = C;
    sr[0][slot] = R;
    __syncthreads();
    for (int stride = 1; stride < L; stride *= 2) {                  // parallel cyclic reduction of the interface system
        const bool lo_in = seg >= stride, hi_in = seg + stride < L;
        const int il = slot - stride, ih = slot + stride;
        const double al = lo_in ? sa[cur][il] : 0.0, bl = lo_in ? sb[cur][il] : 1.0, cl = lo_in ? sc[cur][il] : 0.0, rl = lo_in ? sr[cur][il] : 0.0;
        const double ah = hi_in ? sa[cur][ih] : 0.0, bh = hi_in ? sb[cur][ih] : 1.0, ch = hi_in ? sc[cur][ih] : 0.0, rh = hi_in ? sr[cur][ih] : 0.0;
        const double fl = A / bl, fh = C / bh;
        B = (B - fl * cl) - fh * ah;
        R = (R - fl * rl) - fh * rh;
        A = -(fl * al);
        C = -(fh * ch);
        cur ^= 1;
        sa[cur][slot] = A;
        sb[cur][slot] = B;
        sc[cur][slot] = C;
        sr[cur][slot] = R;
        __syncthreads();
    }
    const double xe = R / B;
    sx[slot] = xe;
    __syncthreads();
    if (!has) return;
    const double xp = seg > 0 ? sx[slot - 1] : 0.0;
    for (int i = s; i < e; ++i) {                                    // pass 3
        const long at = at_of(i);
        z_out[at] = (wy[at] - wv[at] * xp) - ww[at] * xe;
    }
    z_out[at_of(e)] = xe;
}

}  // namespace ccp
