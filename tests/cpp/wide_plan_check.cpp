// Host-only check of the wide pass's segment planner (csrc/ccp_wide_plan.hpp); run by tests/test_wide_plan.py.
//   wide_plan_check plan ROWS TILES_PER_SEGMENT SLOTS T [BORDER_STEPS BORDER_LONGEST]   -> "n_seg h tiles rounds march"
//   wide_plan_check sweep                                 -> "ok CASES" or the first violations, exit status 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

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

// segments of plan p partition [y0, y1): in order, none empty, every boundary at an even distance from y0 when even_h
static void check_partition(const WidePlan &p, int y0, int y1, bool even_h, const char *what)
{
    CHECK(p.n_seg >= 1, "%s rows [%d, %d)", what, y0, y1);
    if (even_h) CHECK(p.h % 2 == 0, "%s h = %d", what, p.h);
    int at = y0;
    for (int s = 0; s < p.n_seg; ++s) {
        int ra, rb;
        wide_segment_rows(y0, y1, p.h, s, ra, rb);
        CHECK(ra == at && rb > ra && rb <= y1, "%s segment %d of %d: [%d, %d), expected start %d, end <= %d", what, s, p.n_seg, ra, rb, at, y1);
        if (even_h) CHECK((ra - y0) % 2 == 0, "%s segment %d starts at %d", what, s, ra);
        if (s + 1 < p.n_seg) CHECK(rb - ra == p.h, "%s segment %d has %d rows, h = %d", what, s, rb - ra, p.h);
        at = rb;
    }
    CHECK(at == y1, "%s ends at %d, not %d", what, at, y1);
}

// the rows of chunk c of the narrow tiling (ccp_fused_plan.hpp, fused_chunk_rows), restated
static void chunk_rows(int st_lo, int st_hi, int first_rows, int last_rows, int R, int n_chunks, int c, int &ra, int &rb)
{
    if (first_rows > 0 && c == 0) {
        ra = st_lo;
        rb = st_lo + first_rows;
    } else if (last_rows > 0 && c == n_chunks - 1) {
        ra = st_hi - last_rows;
        rb = st_hi;
    } else {
        const int k = c - (first_rows > 0 ? 1 : 0);
        const int end = st_hi - last_rows;
        ra = st_lo + first_rows + k * R;
        rb = ra + R < end ? ra + R : end;
    }
}

static long sweep()
{
    long cases = 0;
    const int rows_list[] = {1, 2, 17, 33, 63, 64, 65, 127, 128, 129, 225, 290, 448, 1000, 1023, 4032, 8128, 16320, 16321, 30001};
    const long strips_list[] = {1, 2, 3, 4, 5, 9, 18, 19, 36, 73, 74, 146};
    const int ch_list[] = {1, 2, 3, 4};
    const int slots_list[] = {4, 32, 416, 1024, 1216};
    const int t_list[] = {2, 4, 8};
    for (int rows : rows_list)
        for (int y0 : {0, 1, 32, 33})
            for (long strips : strips_list)
                for (int ch : ch_list)
                    for (int slots : slots_list)
                        for (int T : t_list)
                          for (long bsteps : {0L, 5000L, 66000L}) {
                            const int y1 = y0 + rows;
                            const long tps = strips * ch;
                            WideBorder border;
                            border.steps = bsteps;
                            border.longest = bsteps ? 158 : 0;
                            const WidePlan p = wide_plan(y0, y1, tps, slots, T, border);
                            ++cases;
                            check_partition(p, y0, y1, true, "plan");
                            if (p.n_seg > 1) CHECK(p.h >= kWideMinSegRows, "rows %d: h = %d under the minimum", rows, p.h);
                            // no plan of the same family is cheaper, and none with fewer segments is as cheap
                            const long cost = wide_plan_cost(tps, p.n_seg, p.h, slots, T, border);
                            for (int n = 1; n <= rows / kWideMinSegRows; ++n) {
                                const WidePlan q = wide_plan_count(rows, n);
                                if (q.n_seg != n || (n > 1 && q.h < kWideMinSegRows)) continue;
                                const long c = wide_plan_cost(tps, q.n_seg, q.h, slots, T, border);
                                CHECK(c > cost || (c == cost && q.n_seg >= p.n_seg), "rows %d tiles %ld slots %d: n = %d costs %ld, the plan (n = %d) %ld",
                                      rows, tps, slots, n, c, p.n_seg, cost);
                            }
                        }
    // forced counts: a partition with even boundaries for every n, never more than n segments
    for (int rows : rows_list)
        for (int n : {1, 2, 3, 5, 7, 14, 100, 40000}) {
            const WidePlan p = wide_plan_count(rows, n);
            ++cases;
            check_partition(p, 32, 32 + rows, true, "count");
            CHECK(p.n_seg <= n, "rows %d: %d segments for n = %d", rows, p.n_seg, n);
        }
    // h = R: the interior chunks of the narrow tiling, chunk for chunk
    for (int st_hi : {97, 203, 331, 1536, 4096, 16384})
        for (int R : {16, 31, 32, 48, 64, 140, 364})
            for (int first_rows : {0, 32})
                for (int last_rows : {0, 32})
                    for (int nb_top : {0, 1, 2})
                        for (int nb_bot : {0, 1, 2}) {
                            const int st_lo = 0, mid = st_hi - first_rows - last_rows;
                            if (mid <= 0 || (first_rows > 0 && nb_top == 0) || (last_rows > 0 && nb_bot == 0)) continue;
                            const int n_chunks = (mid + R - 1) / R + (first_rows > 0) + (last_rows > 0);
                            if (nb_top + nb_bot >= n_chunks) continue;
                            int y0, y1, t;
                            chunk_rows(st_lo, st_hi, first_rows, last_rows, R, n_chunks, nb_top, y0, t);
                            chunk_rows(st_lo, st_hi, first_rows, last_rows, R, n_chunks, n_chunks - nb_bot - 1, t, y1);
                            const WidePlan p = wide_plan_height(y1 - y0, R);
                            ++cases;
                            CHECK(p.n_seg == n_chunks - nb_top - nb_bot, "H %d R %d: %d segments for %d interior chunks", st_hi, R, p.n_seg,
                                  n_chunks - nb_top - nb_bot);
                            check_partition(p, y0, y1, false, "height");
                            for (int s = 0; s < p.n_seg; ++s) {
                                int ra, rb, ca, cb;
                                wide_segment_rows(y0, y1, p.h, s, ra, rb);
                                chunk_rows(st_lo, st_hi, first_rows, last_rows, R, n_chunks, nb_top + s, ca, cb);
                                CHECK(ra == ca && rb == cb, "H %d R %d chunk %d: segment [%d, %d), chunk [%d, %d)", st_hi, R, nb_top + s, ra, rb, ca, cb);
                            }
                        }
    return cases;
}

int main(int argc, char **argv)
{
    if ((argc == 6 || argc == 8) && strcmp(argv[1], "plan") == 0) {
        const int rows = atoi(argv[2]), slots = atoi(argv[4]), T = atoi(argv[5]);
        const long tps = atol(argv[3]);
        WideBorder border;
        if (argc == 8) {
            border.steps = atol(argv[6]);
            border.longest = atoi(argv[7]);
        }
        const WidePlan p = wide_plan(32, 32 + rows, tps, slots, T, border);
        const long tiles = tps * p.n_seg;
        printf("%d %d %ld %ld %d\n", p.n_seg, p.h, tiles, (tiles + slots - 1) / slots, wide_march_steps(p.h, T));
        return 0;
    }
    if (argc == 2 && strcmp(argv[1], "sweep") == 0) {
        const long cases = sweep();
        if (failures) {
            printf("%d violations in %ld cases\n", failures, cases);
            return 1;
        }
        printf("ok %ld\n", cases);
        return 0;
    }
    fprintf(stderr, "usage: wide_plan_check plan ROWS TILES_PER_SEGMENT SLOTS T [BORDER_STEPS BORDER_LONGEST] | sweep\n");
    return 2;
}
