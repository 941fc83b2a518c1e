// Host check of the span arithmetic of csrc/ccp_panorama.hpp (span_merge2_chunk, span_merge1_chunk): rows of 1 to 300
// pixels are cut into 64-pixel chunks exactly as k_pano_add's waves cut them -- 64-bit masks of the outer, inner and
// target bytes, early exit once a chain is through -- and the resulting spans are compared with the `first`-based spans
// of lab8_workload.merge_image2 / merge_image, restated serially below.  Built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_panorama_span_host.py; no device is touched.
#include "ccp_panorama.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using Row = std::vector<unsigned char>;

static int W;

template <typename F>
static int first(F cond, int start)
{
    for (int x = start; x < W; ++x)
        if (cond(x)) return x;
    return W;
}

static void ref_merge2(const Row &so, const Row &si, const Row &tg, int *k, int *end)
{
    int a = first([&](int x) { return so[x] != 0; }, 0);
    a = first([&](int x) { return !(si[x] == 0 && tg[x] != 0); }, a);
    *k = a;
    *end = first([&](int x) { return so[x] == 0; }, a);
}

static void ref_merge1(const Row &sm, const Row &tg, int skip, int *k, int *end)
{
    int a = first([&](int x) { return sm[x] != 0; }, 0);
    if (a < W && tg[a] != 0 && skip > 0) a = std::min(W, a + skip);
    *k = a;
    *end = first([&](int x) { return sm[x] == 0; }, a);
}

static uint64_t bits(const Row &r, int base)
{
    uint64_t b = 0;
    for (int i = 0; i < 64 && base + i < W; ++i)
        if (r[(size_t)(base + i)]) b |= 1ull << i;
    return b;
}

static long checked = 0, chunks_saved = 0;

static bool check_row(const Row &so, const Row &si, const Row &tg)
{
    ccp::Span g2 = ccp::span_start(W), m1 = ccp::span_start(W), m0 = ccp::span_start(W);
    bool d2 = false, d1 = false, d0 = false;
    int base = 0;
    for (; base < W && !(d2 && d1 && d0); base += 64) {
        const int n = std::min(64, W - base);
        const uint64_t valid = n == 64 ? ~0ull : (1ull << n) - 1;
        const uint64_t o = bits(so, base), i = bits(si, base), t = bits(tg, base);
        if (!d2) d2 = ccp::span_merge2_chunk(g2, base, valid, o, i, t);
        if (!d1) d1 = ccp::span_merge1_chunk(m1, base, valid, i, t, 1, W);
        if (!d0) d0 = ccp::span_merge1_chunk(m0, base, valid, i, t, 0, W);
    }
    chunks_saved += (W - base + 63) / 64 * (base < W);
    int k, e;
    bool ok = true;
    ref_merge2(so, si, tg, &k, &e);
    // an empty span copies nothing wherever it lies; a non-empty one must match exactly
    auto same = [](const ccp::Span &s, int k_, int e_) { return (s.k >= s.end && k_ >= e_) || (s.k == k_ && s.end == e_); };
    ok &= same(g2, k, e);
    ref_merge1(si, tg, 1, &k, &e);
    ok &= same(m1, k, e);
    ref_merge1(si, tg, 0, &k, &e);
    ok &= same(m0, k, e);
    ok &= g2.k <= W && g2.end <= W && m1.k <= W && m1.end <= W && m0.k <= W && m0.end <= W && g2.k >= 0 && m1.k >= 0 && m0.k >= 0;
    ++checked;
    if (!ok) {
        std::printf("MISMATCH W=%d\n so=", W);
        for (int x = 0; x < W; ++x) std::printf("%d", so[x] != 0);
        std::printf("\n si=");
        for (int x = 0; x < W; ++x) std::printf("%d", si[x] != 0);
        std::printf("\n tg=");
        for (int x = 0; x < W; ++x) std::printf("%d", tg[x] != 0);
        std::printf("\n");
    }
    return ok;
}

int main()
{
    bool ok = true;
    // exhaustive: every outer / inner / target pattern of rows of 1 to 4 pixels
    for (W = 1; W <= 4; ++W)
        for (int a = 0; a < 1 << W; ++a)
            for (int b = 0; b < 1 << W; ++b)
                for (int c = 0; c < 1 << W; ++c) {
                    Row so(W), si(W), tg(W);
                    for (int x = 0; x < W; ++x) {
                        so[x] = (a >> x & 1) * 255;
                        si[x] = (b >> x & 1) * 255;
                        tg[x] = (c >> x & 1) * 255;
                    }
                    ok &= check_row(so, si, tg);
                }
    std::mt19937 gen(2308);
    auto coin = [&](double p) { return std::uniform_real_distribution<double>(0, 1)(gen) < p; };
    for (W = 1; W <= 300; ++W) {
        auto run = [&](Row &r, int a, int b) {
            for (int x = std::max(0, a); x < std::min(W, b); ++x) r[(size_t)x] = 255;
        };
        // the named cases, each with an empty, a full and a random target, and inner equal to, inside and beside outer
        for (int shape = 0; shape < 5; ++shape)
            for (int tgt = 0; tgt < 4; ++tgt)
                for (int inn = 0; inn < 3; ++inn) {
                    Row so(W, 0), si(W, 0), tg(W, 0);
                    int a = 0, b = 0;
                    switch (shape) {
                    case 0: break;                                   // an empty source
                    case 1: a = 0, b = (W + 2) / 3; break;           // a run at column 0
                    case 2: a = W / 2, b = W; break;                 // a run reaching the last column
                    case 3: a = W / 8, b = W / 3; run(so, 2 * W / 3, 2 * W / 3 + W / 5 + 1); run(si, 2 * W / 3, 2 * W / 3 + W / 5 + 1); break;   // two runs
                    default: a = W / 3, b = 2 * W / 3 + 1;           // (the target covers its first pixel below)
                    }
                    run(so, a, b);
                    if (inn == 0) run(si, a, b);
                    if (inn == 1) run(si, a + 2, b - 2);
                    if (inn == 2) run(si, a + (b - a) / 2, b + 3);
                    if (tgt == 1) run(tg, 0, W);
                    if (tgt == 2) for (int x = 0; x < W; ++x) tg[(size_t)x] = coin(0.5) * 255;
                    if (tgt == 3) run(tg, a, a + 1 + W / 7);         // covered at the first source pixel (and a little on)
                    ok &= check_row(so, si, tg);
                }
        for (double p : {0.03, 0.1, 0.5, 0.9, 0.97})
            for (int rep = 0; rep < 6; ++rep) {
                Row so(W), si(W), tg(W);
                for (int x = 0; x < W; ++x) {
                    so[(size_t)x] = coin(p) * 255;
                    si[(size_t)x] = coin(p) * 255 & (rep & 1 ? so[(size_t)x] : 255);
                    tg[(size_t)x] = coin(rep < 3 ? p : 1 - p) * 255;
                }
                ok &= check_row(so, si, tg);
            }
    }
    std::printf("rows checked %ld, chunks skipped by early exit %ld\n", checked, chunks_saved);
    if (chunks_saved == 0) ok = false;                              // the early exit never fired: the drive is wrong
    std::printf(ok ? "spans agree\n" : "FAILED\n");
    return ok ? 0 : 1;
}
