// Runs k_mgl_lines (csrc/ccp_grid_mgl.hpp), the kernel's own source, on the host: a workgroup is 256 threads and a
// barrier (tests/cpp/mgl_host/ccp_grid_mg.hpp).  Every kind of half pass (rows from b alone, rows, columns, columns with
// the prolongation fused), both parities, on shapes with short, long and single-cell lines, with and without dead cells,
// is compared with a serial long double Thomas solve of the same lines: relative max-norm error below 1e-9 (weights span
// 1e-4 .. 1e4), dead cells exactly 0, the other parity's lines untouched.  Built with -fsanitize=address,undefined by
// tests/test_mgl_host.py: every buffer has exactly the level's size, so an index past it is reported.  Exit 0: all good.
#include "ccp_grid_mgl.hpp"
#include <cmath>
#include <random>
#include <thread>
#include <vector>
using namespace ccp;
template <int DIR, bool FIRST, bool ADD>
void launch(int blocks, MgLevel f, const double *b, const double *zin, double *zout, double *wy, double *wv, double *ww, MgLevel c, const double *ec, double cs, int parity, int L)
{
    for (int bx = 0; bx < blocks; ++bx) {
        std::barrier<> bar(kBlock);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (int t = 0; t < kBlock; ++t)
            th.emplace_back([=] { threadIdx = {(unsigned)t, 0, 0}; blockIdx = {(unsigned)bx, 0, 0};
                k_mgl_lines<DIR, FIRST, ADD>(f, b, zin, zout, wy, wv, ww, c, ec, cs, parity, L, nullptr); });
        for (auto &x : th) x.join();
    }
}
struct Lv { int W, H; long pitch; std::vector<double> d, we, ws; MgLevel m; };
int main()
{
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> U(0, 1);
    double worst = 0;
    int shapes[][2] = {{67, 3}, {1, 40}, {40, 1}, {257, 31}, {2053, 5}, {5, 2053}, {33, 34}, {4100, 2}, {2, 4100}, {37, 700}};
    for (auto &sh : shapes) for (int deadmode = 0; deadmode < 2; ++deadmode) {
        const int W = sh[0], H = sh[1];
        const long pitch = (((long)W + 1) / 2 + 15) / 16 * 16, n = (long)H * 2 * pitch;
        const int Wc = (W + 1) / 2, Hc = (H + 1) / 2;
        const long pc = (((long)Wc + 1) / 2 + 15) / 16 * 16, nc = (long)Hc * 2 * pc;
        std::vector<double> d(n, 0), we(n, 0), ws(n, 0), b(n, 0), z(n, 0), t(n, 0), ec(nc, 0), wy(n, 0), wv(n, 0), ww(n, 0);
        std::vector<char> dead((size_t)W * H, 0);
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) if (deadmode && (U(rng) < 0.1 || x == W / 3 || y == H / 3)) dead[(size_t)y * W + x] = 1;
        auto D = [&](int x, int y) { return x < 0 || y < 0 || x >= W || y >= H || dead[(size_t)y * W + x]; };
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            const long a = mg_at(pitch, x, y);
            if (!D(x, y) && !D(x + 1, y)) we[a] = std::pow(10.0, 8 * U(rng) - 4);
            if (!D(x, y) && !D(x, y + 1)) ws[a] = std::pow(10.0, 8 * U(rng) - 4);
        }
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            const long a = mg_at(pitch, x, y);
            if (D(x, y)) continue;
            d[a] = 1.0 + we[a] + ws[a] + (x > 0 ? we[mg_at(pitch, x - 1, y)] : 0) + (y > 0 ? ws[mg_at(pitch, x, y - 1)] : 0);
            b[a] = 100 * (U(rng) - 0.5);
            t[a] = 100 * (U(rng) - 0.5);
        }
        for (int y = 0; y < Hc; ++y) for (int x = 0; x < Wc; ++x) ec[mg_at(pc, x, y)] = U(rng) - 0.5;
        MgLevel f{W, H, pitch, d.data(), we.data(), ws.data(), nullptr, {}, 0, 0, H}, c{Wc, Hc, pc, nullptr, nullptr, nullptr, nullptr, {}, 0, 0, Hc};
        // four kinds of pass, each against a serial long double Thomas on the same inputs
        for (int pass = 0; pass < 4; ++pass) for (int parity = 0; parity < 2; ++parity) {
            const int DIR = pass < 2 ? 0 : 1;
            const bool FIRST = pass == 0, ADD = pass == 3;
            if (FIRST && parity) continue;
            if (ADD && !parity) continue;
            const int nline = DIR == 0 ? W : H, across = DIR == 0 ? H : W;
            const int count = (across - parity + 1) / 2;
            if (count <= 0) continue;
            const int L = mgl_lanes(DIR, nline), per = kBlock / L, blocks = (count + per - 1) / per;
            std::vector<double> zin = t, zout = ADD ? std::vector<double>(n, 777.0) : t;
            const double cs = 2.0;
            if (pass == 0) launch<0, true, false>(blocks, f, b.data(), zout.data(), zout.data(), wy.data(), wv.data(), ww.data(), f, nullptr, 0, parity, L);
            if (pass == 1) launch<0, false, false>(blocks, f, b.data(), zout.data(), zout.data(), wy.data(), wv.data(), ww.data(), f, nullptr, 0, parity, L);
            if (pass == 2) launch<1, false, false>(blocks, f, b.data(), zout.data(), zout.data(), wy.data(), wv.data(), ww.data(), f, nullptr, 0, parity, L);
            if (pass == 3) launch<1, false, true>(blocks, f, b.data(), zin.data(), zout.data(), wy.data(), wv.data(), ww.data(), c, ec.data(), cs, parity, L);
            auto Z = [&](int x, int y) -> long double {
                if (x < 0 || y < 0 || x >= W || y >= H) return 0;
                long double v = t[mg_at(pitch, x, y)];
                if (ADD && !D(x, y)) v += cs * ec[mg_at(pc, x >> 1, y >> 1)];
                return v;
            };
            double scale = 0, err = 0;
            for (int line = parity; line < across; line += 2) {
                std::vector<long double> lo(nline), di(nline), up(nline), r(nline), cp(nline), yy(nline), x(nline);
                for (int i = 0; i < nline; ++i) {
                    const int px = DIR == 0 ? i : line, py = DIR == 0 ? line : i;
                    const long a = mg_at(pitch, px, py);
                    if (D(px, py)) { lo[i] = up[i] = r[i] = 0; di[i] = 1; continue; }
                    di[i] = d[a];
                    up[i] = i + 1 < nline ? -(DIR == 0 ? we[a] : ws[a]) : 0;
                    const int qx = DIR == 0 ? i - 1 : line, qy = DIR == 0 ? line : i - 1;
                    lo[i] = i > 0 ? -(DIR == 0 ? we[mg_at(pitch, qx, qy)] : ws[mg_at(pitch, qx, qy)]) : 0;
                    r[i] = b[a];
                    if (!FIRST) {
                        if (DIR == 0) r[i] += (py > 0 ? ws[mg_at(pitch, px, py - 1)] : 0) * Z(px, py - 1) + ws[a] * Z(px, py + 1);
                        else r[i] += (px > 0 ? we[mg_at(pitch, px - 1, py)] : 0) * Z(px - 1, py) + we[a] * Z(px + 1, py);
                    }
                }
                cp[0] = up[0] / di[0]; yy[0] = r[0] / di[0];
                for (int i = 1; i < nline; ++i) { long double den = di[i] - lo[i] * cp[i - 1]; cp[i] = up[i] / den; yy[i] = (r[i] - lo[i] * yy[i - 1]) / den; }
                x[nline - 1] = yy[nline - 1];
                for (int i = nline - 2; i >= 0; --i) x[i] = yy[i] - cp[i] * x[i + 1];
                for (int i = 0; i < nline; ++i) {
                    const int px = DIR == 0 ? i : line, py = DIR == 0 ? line : i;
                    const double got = zout[mg_at(pitch, px, py)];
                    if (D(px, py) && got != 0.0) { std::printf("dead cell not 0 at %d %d\n", px, py); return 1; }
                    scale = std::max(scale, (double)fabsl(x[i]));
                    err = std::max(err, (double)fabsl(got - x[i]));
                }
            }
            // the other parity's lines and the pads are untouched
            const std::vector<double> &ref = ADD ? std::vector<double>(n, 777.0) : t;
            for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
                const int line = DIR == 0 ? y : x;
                if ((line & 1) != parity && zout[mg_at(pitch, x, y)] != ref[mg_at(pitch, x, y)]) { std::printf("other parity written\n"); return 1; }
            }
            const double rel = scale > 0 ? err / scale : err;
            worst = std::max(worst, rel);
            std::printf("%dx%d dead=%d pass=%d parity=%d L=%d blocks=%d rel err %.2e\n", W, H, deadmode, pass, parity, L, blocks, rel);
            if (!(rel < 1e-9)) return 1;
        }
    }
    std::printf("worst %.2e\n", worst);
    return 0;
}
