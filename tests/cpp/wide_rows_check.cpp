// Host-only check of how a wide tile addresses its rows (csrc/ccp_wide_plan.hpp: wide_march, wide_turn_rows,
// wide_row_offset, wide_rows_stride_ok); run by tests/test_wide_rows.py.
//   wide_rows_check sweep   -> "ok CASES" or the first violations, exit status 1
//
// The range check of a raw buffer instruction is modelled as the hardware states it: an access of 16 bytes at byte
// offset `off` (32 bits, the lane's offset plus the row's) from the descriptor's base is performed iff
// off + 16 <= num_records.  The sums are formed in 64 bits here and must stay below 2^32: nothing may depend on a wrap.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ccp_wide_plan.hpp"

using namespace ccp;

static int failures = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                printf("FAIL %s: ", #cond);               \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

constexpr int T = 8;
constexpr uint32_t kLaneOut = 0x80000000u;     // ccp_grid_fused.hpp: the offset of a lane whose columns do not exist

// does the access of the window's k-th row by a lane at `lane` bytes into the row (or kLaneOut) go through, and where
static bool performed(const WideTurnRows &w, int k, uint32_t stride, uint32_t lane, int &row)
{
    const uint64_t off = (uint64_t)wide_row_offset(k, w.skip, stride) + lane;
    CHECK(off + 16 <= 0xffffffffull, "offset wraps: k %d skip %d stride %u lane %u", k, w.skip, stride, lane);
    const bool in = off + 16 <= w.records;
    if (in) {
        CHECK(off < 0x80000000ull, "offset %llu of a performed access", (unsigned long long)off);
        row = w.first + (int)(off / stride);
        CHECK(off % stride == lane, "offset %llu is not in the lane's columns", (unsigned long long)off);
    }
    return in;
}

// one window against the rows [lo, hi) that exist; marks the rows it reaches in `hits`
static void check_window(const char *what, int w0, int lo, int hi, uint32_t stride, bool lanes, std::vector<int> &hits, int origin)
{
    const WideTurnRows w = wide_turn_rows(w0, lo, hi, stride);
    CHECK(w.records <= kWideRowOut, "%s window %d: records %u", what, w0, w.records);
    CHECK(w.records % stride == 0 && w.records / stride <= (uint32_t)kWideRing, "%s window %d: records %u", what, w0, w.records);
    for (int k = 0; k < kWideRing; ++k) {
        const int q = w0 + k;
        const bool want = q >= lo && q < hi;
        int row = 0;
        const bool got = performed(w, k, stride, 0, row);
        CHECK(got == want, "%s window %d rows [%d, %d): row %d %s", what, w0, lo, hi, q, got ? "is reached" : "is dropped");
        if (got) {
            CHECK(row == q, "%s window %d: row %d lands on row %d", what, w0, q, row);
            hits[(size_t)(q - origin)]++;
        } else {
            // "an offset at or beyond num_records, or num_records = 0"
            CHECK(w.records == 0 || wide_row_offset(k, w.skip, stride) >= w.records, "%s window %d row %d", what, w0, q);
        }
        if (lanes) {
            CHECK(performed(w, k, stride, stride - 16, row) == want && (!want || row == q), "%s window %d row %d, last lane", what, w0, q);
            CHECK(!performed(w, k, stride, kLaneOut, row), "%s window %d row %d: a lane that is out is reached", what, w0, q);
        }
    }
    // the rows either side of the window are not part of it: whatever k would reach them is never formed, and the
    // descriptor does not cover them either
    CHECK((uint64_t)w.records <= (uint64_t)kWideRing * stride, "%s window %d covers rows past its end", what, w0);
}

static long sweep()
{
    long cases = 0;
    const uint32_t strides[] = {16u, 4096u, 16384u * 8u, (uint32_t)(kWideRowOut / kWideRowSpan) & ~15u};
    for (int local_rows = 1; local_rows <= 120; ++local_rows)
        for (int ra = 0; ra < local_rows; ++ra)
            for (int rb = ra + 1; rb <= local_rows; ++rb)
                for (int y0 = 0; y0 < 2; ++y0) {
                    const WideMarch m = wide_march(ra, rb, local_rows, y0, T);
                    CHECK(m.m0 >= 0 && m.m0 <= ra && m.m1 >= rb && m.m1 <= local_rows, "march [%d, %d) of %d", ra, rb, local_rows);
                    CHECK(m.base == m.m0 || m.base == m.m0 - 1, "base %d, m0 %d", m.base, m.m0);
                    CHECK(((y0 + m.base) & 1) == 0, "base %d is an odd image row", m.base);
                    const bool lanes = (cases % 64) == 0;
                    const uint32_t stride = strides[cases % 4];
                    const int origin = -2 * T - 2;
                    std::vector<int> loaded((size_t)(local_rows + 8 * T + 2 * kWideRing + 8), 0), stored(loaded.size(), 0);
                    // the rows the march starts with, before its first turn, have a descriptor each
                    for (int q = m.base; q < m.base + kWideLoadAhead; ++q)
                        if (q >= m.m0 && q < m.m1) loaded[(size_t)(q - origin)]++;
                    for (int fb = m.base; fb <= m.f_end; fb += kWideRing) {
                        const int wl = fb + kWideLoadAhead, ws = fb - 2 * T;
                        CHECK(wide_turn_rows(wl, m.m0, m.m1, stride).skip == 0, "a turn loads row %d before m0 = %d", wl, m.m0);
                        check_window("load", wl, m.m0, m.m1, stride, lanes, loaded, origin);
                        check_window("store", ws, ra, rb, stride, lanes, stored, origin);
                    }
                    for (int q = origin; q < origin + (int)loaded.size(); ++q) {
                        const int nl = loaded[(size_t)(q - origin)], ns = stored[(size_t)(q - origin)];
                        CHECK(nl == (q >= m.m0 && q < m.m1 ? 1 : 0), "[%d, %d) of %d, y0 %d: row %d loaded %d times", ra, rb, local_rows, y0, q, nl);
                        CHECK(ns == (q >= ra && q < rb ? 1 : 0), "[%d, %d) of %d, y0 %d: row %d stored %d times", ra, rb, local_rows, y0, q, ns);
                    }
                    ++cases;
                }
    // windows far from the rows that exist, on either side, and empty row ranges
    for (int w0 = -100; w0 <= 100; ++w0)
        for (int lo = -3; lo <= 30; lo += 3)
            for (int hi = lo; hi <= lo + 45; hi += 5) {
                std::vector<int> hits(400, 0);
                check_window("free", w0, lo, hi, 4096u, true, hits, -150);
                ++cases;
            }
    // a forced single segment of the headline: 16,320 rows of 128 KB, 4 GB of plane; offsets restart every turn
    {
        const uint32_t stride = 16384u * 8u;
        const WideMarch m = wide_march(32, 16352, 16384, 0, T);
        std::vector<int> loaded(16384 + 200, 0), stored(loaded.size(), 0);
        for (int fb = m.base; fb <= m.f_end; fb += kWideRing) {
            check_window("load", fb + kWideLoadAhead, m.m0, m.m1, stride, true, loaded, -100);
            check_window("store", fb - 2 * T, 32, 16352, stride, true, stored, -100);
        }
        for (int q = 32; q < 16352; ++q) CHECK(stored[(size_t)(q + 100)] == 1, "row %d stored %d times", q, stored[(size_t)(q + 100)]);
        ++cases;
    }
    // the guard: every offset the march forms is below (kWideRing + 4) strides, and the guard refuses a stride for which
    // that reaches 2^31 — and already one for which it passes kWideRowOut, so that kWideRowOut is beyond every descriptor
    // and a lane that is out (2^31) plus any row offset stays below 2^32
    const long limit = (long)(kWideRowOut / kWideRowSpan);
    CHECK(wide_rows_stride_ok(16) && wide_rows_stride_ok(16384L * 8) && wide_rows_stride_ok(limit), "strides in range");
    CHECK(!wide_rows_stride_ok(-16) && !wide_rows_stride_ok(limit + 1), "strides out of range");
    CHECK(!wide_rows_stride_ok(((1L << 31) + kWideRowSpan - 1) / kWideRowSpan), "the bound reaches 2^31");
    CHECK(!wide_rows_stride_ok(1L << 31) && !wide_rows_stride_ok(1L << 33), "beyond 32 bits");
    CHECK((uint64_t)limit * kWideRowSpan <= kWideRowOut, "the guard's own bound");
    CHECK((uint64_t)kLaneOut + (uint64_t)limit * kWideRowSpan + 16 <= 0xffffffffull, "a lane that is out wraps");
    CHECK((uint64_t)kLaneOut + kWideRowOut + 16 <= 0xffffffffull, "a lane that is out in a row that is out wraps");
    return cases;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        const long cases = sweep();
        if (failures) {
            printf("%d violations\n", failures);
            return 1;
        }
        printf("ok %ld\n", cases);
        return 0;
    }
    fprintf(stderr, "usage: wide_rows_check sweep\n");
    return 2;
}
