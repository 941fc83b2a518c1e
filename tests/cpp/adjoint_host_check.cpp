// adjoint_host_check.cpp — csrc/ccp_grid_adjoint.hpp's two pixel bodies run on the host (CCP_ADJOINT_HOST) under
// AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_adjoint_host.py builds and runs this).  Every buffer is a heap
// array of exactly its view's size -- one past the last element the view can reach -- so an index that leaves its view
// leaves its allocation.  The results are compared, exactly, with a plain raster-order restatement of the header's
// formulas on natural-order arrays.  Shapes: those of tests/test_gpu_adjoint.py, the one-pixel-wide and -tall ones
// included; C = 1 and 3; no, some and all pixels fixed; every input present or absent; F64 and F32 outputs;
// interleaved and planar output views; all outputs and a few.
#define CCP_ADJOINT_HOST
#include "ccp_grid_adjoint.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace ccp;

static unsigned long long rng_state = 88172645463325252ull;
static double uniform(double lo, double hi)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return lo + (hi - lo) * (double)(rng_state >> 11) / 9007199254740992.0;
}

template <typename T>
struct Buf {
    std::unique_ptr<T[]> p;
    long n = 0;
    void make(long count) { n = count; p.reset(new T[count]); }
};

// an H x W x C natural array of T with exact size: interleaved (planar == false) or channel-planar
template <typename T>
struct Image {
    Buf<T> b;
    long sy, sx, sc;
    void make(int H, int W, int C, bool planar, double lo, double hi, bool integers = false)
    {
        if (planar) { sc = (long)H * W; sy = W; sx = 1; } else { sy = (long)W * C; sx = C; sc = 1; }
        b.make((long)H * W * C);
        for (long i = 0; i < b.n; ++i) b.p[i] = integers ? (T)(int)uniform(lo, hi) : (T)uniform(lo, hi);
    }
    T &at(int y, int x, int c) { return b.p[y * sy + x * sx + c * sc]; }
    AdjIn in(int dtype) const { return AdjIn{b.p.get(), sy, sx, sc, dtype}; }
    AdjOut out(int dtype) const { return AdjOut{b.p.get(), sy, sx, sc, dtype}; }
};

static long failures = 0, checked = 0;
static void expect(bool ok, const char *what, int W, int H, int C, int variant)
{
    ++checked;
    if (!ok && failures++ < 20) std::printf("MISMATCH %s at %dx%dx%d variant %d\n", what, W, H, C, variant);
}

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same(float a, double b) { const float r = (float)b; return std::memcmp(&a, &r, sizeof a) == 0; }

// fixed: 0 none, 1 about 10 % in runs and on the border, 2 all.  variant bit 0: gx, gy, f, wx, wy, lambda absent; bit 1: F32
// outputs (and an F32 grad, a u8 f, F32 weights, an F32 mask); bit 2: planar outputs; bit 3: only g_wx, g_f, g_values asked for.
template <typename O, typename WT, typename FT, typename GT, typename MT>
static void run_case(int W, int H, int C, int fixed_kind, int variant)
{
    const bool absent = variant & 1, f32 = variant & 2, planar = variant & 4, few = variant & 8;
    const int odt = f32 ? kAdjF32 : kAdjF64;
    const long pitch = (((W + 1) / 2 + 15) / 16) * 16, ch_stride = (long)H * 2 * pitch;
    Buf<double> x, b, d;
    x.make(C * ch_stride);
    b.make(C * ch_stride);
    d.make(ch_stride);
    for (long i = 0; i < x.n; ++i) x.p[i] = uniform(-3, 3);
    for (long i = 0; i < b.n; ++i) b.p[i] = 7.0;
    for (long i = 0; i < d.n; ++i) d.p[i] = uniform(0, 1) < 0.2 ? 0.0 : 1.0;
    Image<double> u;
    Image<GT> grad;
    Image<float> gx, gy;
    Image<FT> f;
    Image<WT> wx, wy, lam;
    Image<MT> fixed;
    u.make(H, W, C, false, -2, 2);
    grad.make(H, W, C, planar, -1, 1);
    gx.make(H, W, C, false, -1, 1);
    gy.make(H, W, C, true, -1, 1);
    f.make(H, W, C, false, 0, 255, sizeof(FT) == 1);
    wx.make(H, W, 1, false, 0.1, 10);
    wy.make(H, W, 1, false, 0.1, 10);
    lam.make(H, W, 1, false, 0, 1);
    fixed.make(H, W, 1, false, 0, 0);
    for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) {
            bool fx = fixed_kind == 2;
            if (fixed_kind == 1) fx = (xx == 0 && y % 3 == 0) || (y == H - 1 && xx % 4 < 2) || ((xx * 7 + y * 13) % 23 == 0);
            fixed.at(y, xx, 0) = fx ? (MT)1 : (MT)0;
        }
    Image<O> o_wx, o_wy, o_lam, o_gx, o_gy, o_f, o_val;
    o_wx.make(H, W, 1, false, 9, 9);
    o_wy.make(H, W, 1, false, 9, 9);
    o_lam.make(H, W, 1, false, 9, 9);
    o_gx.make(H, W, C, planar, 9, 9);
    o_gy.make(H, W, C, planar, 9, 9);
    o_f.make(H, W, C, planar, 9, 9);
    o_val.make(H, W, C, planar, 9, 9);

    AdjointArgs a{};
    a.v = x.p.get();
    a.pitch = pitch;
    a.ch_stride = ch_stride;
    a.W = W;
    a.H = H;
    a.C = C;
    const int wdt = sizeof(WT) == 8 ? kAdjF64 : kAdjF32, fdt = sizeof(FT) == 1 ? kAdjU8 : sizeof(FT) == 4 ? kAdjF32 : kAdjF64;
    const int gdt = sizeof(GT) == 8 ? kAdjF64 : kAdjF32, mdt = sizeof(MT) == 1 ? kAdjU8 : kAdjF32;
    const AdjIn none{nullptr, 0, 0, 0, 0};
    a.u = u.in(kAdjF64);
    a.grad = grad.in(gdt);
    a.gx = absent ? none : gx.in(kAdjF32);
    a.gy = absent ? none : gy.in(kAdjF32);
    a.f = absent ? none : f.in(fdt);
    a.wx = absent ? none : wx.in(wdt);
    a.wy = absent ? none : wy.in(wdt);
    a.lam = absent ? none : lam.in(wdt);
    a.fixed = fixed_kind == 0 && absent ? none : fixed.in(mdt);
    const AdjOut no{nullptr, 0, 0, 0, 0};
    a.g_wx = o_wx.out(odt);
    a.g_wy = few ? no : o_wy.out(odt);
    a.g_lam = few ? no : o_lam.out(odt);
    a.g_gx = few ? no : o_gx.out(odt);
    a.g_gy = few ? no : o_gy.out(odt);
    a.g_f = o_f.out(odt);
    a.g_val = o_val.out(odt);
    for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) adjoint_pixel(&a, xx, y);

    // the restatement: natural-order v, plain loops
    auto V = [&](int y, int xx, int c) { return fixed.at(y, xx, 0) != 0 ? 0.0 : x.p[c * ch_stride + ((long)y * 2 + ((xx + y) & 1)) * pitch + (xx >> 1)]; };
    auto GX = [&](int y, int xx, int c) { return absent ? 0.0 : (double)gx.at(y, xx, c); };
    auto GY = [&](int y, int xx, int c) { return absent ? 0.0 : (double)gy.at(y, xx, c); };
    auto F = [&](int y, int xx, int c) { return absent ? 0.0 : (double)f.at(y, xx, c); };
    auto WX = [&](int y, int xx) { return absent ? 1.0 : (double)wx.at(y, xx, 0); };
    auto WY = [&](int y, int xx) { return absent ? 1.0 : (double)wy.at(y, xx, 0); };
    for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) {
            const bool fp = fixed.at(y, xx, 0) != 0;
            double ax = 0.0, ay = 0.0, al = 0.0;
            for (int c = 0; c < C; ++c) {
                double ggx = 0.0, ggy = 0.0, gf = 0.0, gv = 0.0;
                if (xx + 1 < W) {
                    const double s = V(y, xx + 1, c) - V(y, xx, c), r = GX(y, xx, c) - (u.at(y, xx + 1, c) - u.at(y, xx, c));
                    ggx = WX(y, xx) * s;
                    ax += s * r;
                }
                if (y + 1 < H) {
                    const double s = V(y + 1, xx, c) - V(y, xx, c), r = GY(y, xx, c) - (u.at(y + 1, xx, c) - u.at(y, xx, c));
                    ggy = WY(y, xx) * s;
                    ay += s * r;
                }
                if (!fp) {
                    gf = (absent ? 0.0 : (double)lam.at(y, xx, 0)) * V(y, xx, c);
                    al += V(y, xx, c) * (F(y, xx, c) - u.at(y, xx, c));
                } else {
                    double t = (double)grad.at(y, xx, c);
                    if (y >= 1) t += WY(y - 1, xx) * V(y - 1, xx, c);
                    if (xx >= 1) t += WX(y, xx - 1) * V(y, xx - 1, c);
                    if (xx + 1 < W) t += WX(y, xx) * V(y, xx + 1, c);
                    if (y + 1 < H) t += WY(y, xx) * V(y + 1, xx, c);
                    gv = t;
                }
                expect(same(o_gx.at(y, xx, c), few ? 9.0 : ggx), "g_gx", W, H, C, variant);
                expect(same(o_gy.at(y, xx, c), few ? 9.0 : ggy), "g_gy", W, H, C, variant);
                expect(same(o_f.at(y, xx, c), gf), "g_f", W, H, C, variant);
                expect(same(o_val.at(y, xx, c), gv), "g_values", W, H, C, variant);
            }
            expect(same(o_wx.at(y, xx, 0), ax), "g_wx", W, H, C, variant);
            expect(same(o_wy.at(y, xx, 0), few ? 9.0 : ay), "g_wy", W, H, C, variant);
            expect(same(o_lam.at(y, xx, 0), few ? 9.0 : (fp ? 0.0 : al)), "g_lambda", W, H, C, variant);
        }

    // ccp_grid_adjoint_begin_device's body
    for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) adjoint_begin_pixel(b.p.get(), x.p.get(), d.p.get(), pitch, ch_stride, C, grad.in(gdt), xx, y);
    for (int c = 0; c < C; ++c)
        for (int y = 0; y < H; ++y)
            for (int xx = 0; xx < W; ++xx) {
                const long at = ((long)y * 2 + ((xx + y) & 1)) * pitch + (xx >> 1);
                expect(same(b.p[c * ch_stride + at], d.p[at] != 0.0 ? (double)grad.at(y, xx, c) : 0.0), "begin b", W, H, C, variant);
                expect(same(x.p[c * ch_stride + at], 0.0), "begin x", W, H, C, variant);
            }
}

int main()
{
    const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {33, 17}, {70, 40}, {257, 131}};
    for (const auto &s : shapes)
        for (int C : {1, 3})
            for (int fixed_kind = 0; fixed_kind < 3; ++fixed_kind)
                for (int variant = 0; variant < 16; ++variant) {
                    if ((long)s[0] * s[1] > 5000 && variant != 0 && variant != 6 && variant != 9 && variant != 15) continue;   // the largest shape: four variants
                    if (variant & 2)
                        run_case<float, float, unsigned char, float, float>(s[0], s[1], C, fixed_kind, variant);
                    else
                        run_case<double, double, double, double, unsigned char>(s[0], s[1], C, fixed_kind, variant);
                }
    std::printf("checked %ld values, %ld mismatches\n", checked, failures);
    return failures ? 1 : 0;
}
