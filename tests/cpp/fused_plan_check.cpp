// Host-only check of the red-black pass planner (csrc/ccp_fused_plan.hpp); run by tests/test_fused_plan.py.
//   fused_plan_check batch   reads one pass per line from stdin:
//       W H C y0 local_rows own_lo own_hi ghost ghost_top ghost_bottom send_up send_down R T cus since k
//       l1 edge_rows masked multi short_edges all_border side_rows_override wide wide_segments
//     (the pass is pass k, from 0, of a run of depth-T passes that starts `since` half-sweeps after a halo refresh), checks
//     the plan's invariants and prints its fields as "name=value ..."; a line "skip" where the ghosts are exhausted or
//     no row is left to store.  Violations are printed as "FAIL ..." lines, exit status 1.
//   fused_plan_check splits  sweeps fused_pass_split and fused_stores_red -> "ok CASES" or the first violations
//   fused_plan_check split ITERATIONS TMAX FREE [COST_1 .. COST_TMAX]   -> "in_place free_parity depth depth ..."
//   fused_plan_check tune W H y0 local_rows C T SLOTS   -> the chunk heights ccp_grid_tune would time
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "ccp_fused_plan.hpp"

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

// rows covered so far of one (chunk, strip) tile, by which launch
struct Cover {
    int next = -1;        // the next row a tile of this (chunk, strip) must start at
    int ordinary = 0, border = 0;
};

// the tile rule of k_fused_sweep, restated
static bool is_border_tile(const FusedPlan &P, int chunk, int sx)
{
    return chunk < P.nb_top || chunk >= P.n_chunks - P.nb_bot || sx < P.ns_left || sx >= P.n_strips - P.ns_right;
}

static void check_plan(const FusedPlanInput &in, const FusedPassKind &kind, const FusedPlan &P, long line)
{
    const int T = P.T, U = fused_useful_px(T);
    // chunks partition [st_lo, st_hi) in order
    int at = P.st_lo;
    for (int c = 0; c < P.n_chunks; ++c) {
        int ra, rb;
        fused_chunk_rows(P, c, ra, rb);
        CHECK(ra == at && rb > ra, "line %ld chunk %d of %d: [%d, %d), expected start %d", line, c, P.n_chunks, ra, rb, at);
        at = rb;
    }
    CHECK(at == P.st_hi, "line %ld: chunks end at %d, st_hi %d", line, at, P.st_hi);
    CHECK(P.n_strips * U >= in.g.W && (P.n_strips - 1) * U < in.g.W, "line %ld: %d strips for W %d", line, P.n_strips, in.g.W);
    // fused_chunk_of: a bijection of [0, n_chunks), the edge chunks first
    std::vector<int> seen(P.n_chunks, 0);
    const int n_e = P.first_edge + P.last_edge;
    for (int y = 0; y < P.n_chunks; ++y) {
        const int c = fused_chunk_of(P, y);
        CHECK(c >= 0 && c < P.n_chunks, "line %ld: chunk_of(%d) = %d", line, y, c);
        if (c < 0 || c >= P.n_chunks) continue;
        seen[c]++;
        CHECK(fused_is_edge_chunk(P, c) == (y < n_e), "line %ld: chunk_of(%d) = %d, %d edge chunks", line, y, c, n_e);
    }
    for (int c = 0; c < P.n_chunks; ++c) CHECK(seen[c] == 1, "line %ld: chunk %d dispatched %d times", line, c, seen[c]);
    CHECK(P.edge || P.edge_target == 0, "line %ld: target without an edge pass", line);
    if (!P.edge) CHECK(kind.edge_rows == 0 || n_e == 0, "line %ld: edge chunks in a pass that does not signal", line);

    // every (chunk, strip) tile in exactly one of the two launches; side sub-tiles partition their chunk
    std::map<std::pair<int, int>, Cover> cover;
    long edge_waves = 0;
    auto take = [&](int chunk, int sx, int ra, int rb, bool border) {
        if (ra >= rb) return;                                          // (the kernels' waves leave at once)
        int c0, c1;
        fused_chunk_rows(P, chunk, c0, c1);
        Cover &cv = cover[{chunk, sx}];
        if (cv.next < 0) cv.next = c0;
        CHECK(ra == cv.next && rb <= c1, "line %ld tile (%d, %d): rows [%d, %d) after %d in chunk [%d, %d)", line, chunk, sx, ra, rb, cv.next, c0, c1);
        cv.next = rb;
        (border ? cv.border : cv.ordinary)++;
        if (P.edge && fused_is_edge_chunk(P, chunk)) ++edge_waves;
    };
    if (P.any_plain)
        for (unsigned by = 0; by < P.grid_y; ++by)
            for (unsigned w = 0; w < P.grid_x * kTileWaves; ++w) {
                const int sx = (int)w, chunk = P.edge ? fused_chunk_of(P, (int)by) : (int)by;
                if (sx >= P.n_strips || (!kind.masked && is_border_tile(P, chunk, sx))) continue;
                int ra, rb;
                fused_chunk_rows(P, chunk, ra, rb);
                take(chunk, sx, ra, rb, false);
            }
    {   // the border launch's tile ids, as k_fused_border decodes them
        const int inner = P.n_strips - P.edge_strips;
        const long n_full = (long)P.edge_chunks * inner, n_side = (long)P.n_chunks * P.edge_strips * P.side_subs;
        CHECK(kind.masked ? P.n_border == 0 : P.n_border == n_full + n_side, "line %ld: n_border %ld, %ld + %ld", line, P.n_border, n_full, n_side);
        CHECK((long)P.bgrid_x * kTileWaves >= P.n_border && ((long)P.bgrid_x - 1) * kTileWaves < P.n_border, "line %ld: border grid %u for %ld tiles",
              line, P.bgrid_x, P.n_border);
        for (long id = 0; id < P.n_border; ++id) {
            int chunk, sx, ra, rb;
            if (id < n_full) {
                const int e = (int)(id / inner);
                sx = P.ns_left + (int)(id % inner);
                chunk = e < P.nb_top ? e : P.n_chunks - P.edge_chunks + e;
                fused_chunk_rows(P, chunk, ra, rb);
            } else {
                long k = id - n_full;
                const int sub = (int)(k % P.side_subs);
                k /= P.side_subs;
                const int e = (int)(k % P.edge_strips);
                chunk = P.edge ? fused_chunk_of(P, (int)(k / P.edge_strips)) : (int)(k / P.edge_strips);
                sx = e < P.ns_left ? e : P.n_strips - P.edge_strips + e;
                int c0, c1;
                fused_chunk_rows(P, chunk, c0, c1);
                const int sr = (P.edge && fused_is_edge_chunk(P, chunk)) ? P.side_rows_edge : P.side_rows;
                ra = c0 + sub * sr;
                rb = ra + sr < c1 ? ra + sr : c1;
            }
            CHECK(is_border_tile(P, chunk, sx), "line %ld: border id %ld is the ordinary tile (%d, %d)", line, id, chunk, sx);
            take(chunk, sx, ra, rb, true);
        }
    }
    for (int c = 0; c < P.n_chunks; ++c)
        for (int s = 0; s < P.n_strips; ++s) {
            int c0, c1;
            fused_chunk_rows(P, c, c0, c1);
            const Cover cv = cover.count({c, s}) ? cover[{c, s}] : Cover();
            CHECK(cv.next == c1, "line %ld tile (%d, %d): covered to %d of [%d, %d)", line, c, s, cv.next, c0, c1);
            CHECK((cv.ordinary == 1 && cv.border == 0) || (cv.ordinary == 0 && cv.border >= 1), "line %ld tile (%d, %d): %d ordinary, %d border tiles",
                  line, c, s, cv.ordinary, cv.border);
        }
    CHECK(P.edge_target == (unsigned long long)edge_waves * P.channels, "line %ld: edge_target %llu, %ld waves x %d channels", line, P.edge_target,
          edge_waves, P.channels);
    CHECK(P.grid_y == (unsigned)P.n_chunks && (int)P.grid_x * kTileWaves >= P.n_strips && ((int)P.grid_x - 1) * kTileWaves < P.n_strips,
          "line %ld: grid %u x %u for %d strips x %d chunks", line, P.grid_x, P.grid_y, P.n_strips, P.n_chunks);

    // the wide tiles cover exactly the pixels the ordinary narrow tiles would store, each once
    if (P.wide) {
        CHECK(T == kWideT && kind.l1 == 0 && !P.edge && in.wide && !kind.masked && !kind.multi, "line %ld: a wide pass of the wrong kind", line);
        const int WU = wide_useful_px(T);
        std::vector<int> cols(in.g.W + 2 * WU, 0), rows(in.g.local_rows + 1, 0);
        for (int sw = 0; sw < P.n_wide; ++sw)
            for (int x = P.wx0 + sw * WU; x < std::min(P.wx0 + sw * WU + WU, P.wx1); ++x) cols[x]++;
        for (int s = P.ns_left; s < P.n_strips - P.ns_right; ++s)
            for (int x = s * U; x < (s + 1) * U; ++x) cols[x]--;       // (inner strips end before the last column)
        for (size_t x = 0; x < cols.size(); ++x) CHECK(cols[x] == 0, "line %ld column %zu: wide - narrow = %d", line, x, cols[x]);
        CHECK(P.wx1 <= in.g.W && P.wx0 >= 0 && P.wx0 % 2 == 0, "line %ld: wide columns [%d, %d) of %d", line, P.wx0, P.wx1, in.g.W);
        for (int s = 0; s < P.wide_nseg; ++s) {
            int ra, rb;
            wide_segment_rows(P.wide_y0, P.wide_y1, P.wide_h, s, ra, rb);
            CHECK(rb > ra, "line %ld: segment %d is empty", line, s);
            for (int y = ra; y < rb; ++y) rows[y]++;
        }
        for (int c = P.nb_top; c < P.n_chunks - P.nb_bot; ++c) {
            int ra, rb;
            fused_chunk_rows(P, c, ra, rb);
            for (int y = ra; y < rb; ++y) rows[y]--;
        }
        for (size_t y = 0; y < rows.size(); ++y) CHECK(rows[y] == 0, "line %ld row %zu: wide - narrow = %d", line, y, rows[y]);
        CHECK(P.wide_stride >= P.n_wide && P.wide_tiles == P.wide_stride * P.wide_nseg * P.channels, "line %ld: %d wide tiles", line, P.wide_tiles);
        CHECK((long)P.wgrid_x * kWideWaves >= P.wide_tiles && ((long)P.wgrid_x - 1) * kWideWaves < P.wide_tiles, "line %ld: wide grid %u", line, P.wgrid_x);
    } else {
        CHECK(P.wide_tiles == 0 && P.wgrid_x == 0, "line %ld: wide tiles in a narrow pass", line);
    }
}

// the rows pass 0, 1, ... of a run store: never short of the owned rows, 2T fewer per pass on a stale side only
static void check_stored_rows(const FusedPlanInput &in, int since, int T, long line)
{
    int plo = 0, phi = 0;
    for (int k = 0; !fused_ghosts_exhausted(in, since + 2 * T * (k + 1)); ++k) {
        int lo, hi;
        fused_stored_rows(in, since + 2 * T * (k + 1), lo, hi);
        CHECK(lo >= 0 && lo <= in.g.own_lo && hi >= in.g.own_hi && hi <= in.g.local_rows, "line %ld pass %d: rows [%d, %d), owned [%d, %d)", line, k, lo,
              hi, in.g.own_lo, in.g.own_hi);
        if (!in.stale_top) CHECK(lo == 0, "line %ld pass %d: lo %d at the image top", line, k, lo);
        if (!in.stale_bottom) CHECK(hi == in.g.local_rows, "line %ld pass %d: hi %d at the image bottom", line, k, hi);
        if (k > 0) {
            if (in.stale_top) CHECK(lo == std::min(plo + 2 * T, in.g.own_lo), "line %ld pass %d: lo %d after %d", line, k, lo, plo);
            if (in.stale_bottom) CHECK(hi == std::max(phi - 2 * T, in.g.own_hi), "line %ld pass %d: hi %d after %d", line, k, hi, phi);
        }
        plo = lo;
        phi = hi;
        if (!in.stale_top && !in.stale_bottom) break;                  // (a whole image never runs out)
    }
}

static int batch()
{
    char buf[1024];
    long line = 0;
    while (fgets(buf, sizeof(buf), stdin)) {
        ++line;
        int v[26];
        int n = 0;
        for (char *tok = strtok(buf, " \n"); tok && n < 26; tok = strtok(nullptr, " \n")) v[n++] = atoi(tok);
        if (n != 26) {
            printf("FAIL line %ld: %d fields\n", line, n);
            return 1;
        }
        FusedPlanInput in;
        in.g.W = v[0];
        in.g.H = v[1];
        in.channels = v[2];
        in.g.y0 = v[3];
        in.g.local_rows = v[4];
        in.g.own_lo = v[5];
        in.g.own_hi = v[6];
        in.g.pitch = in.g.ch_stride = 0;
        in.stale_top = in.g.y0 > 0;
        in.stale_bottom = in.g.y0 + in.g.local_rows < in.g.H;
        in.ghost = v[7];
        in.ghost_top = v[8];
        in.ghost_bottom = v[9];
        in.send_up = v[10];
        in.send_down = v[11];
        in.rows_per_chunk = v[12];
        const int T = v[13];
        in.cus = v[14];
        const int since = v[15], k = v[16];
        FusedPassKind kind;
        kind.T = T;
        kind.l1 = v[17];
        kind.edge_rows = v[18];
        kind.masked = v[19] != 0;
        kind.multi = v[20] != 0;
        in.short_edges = v[21] != 0;
        in.all_border = v[22] != 0;
        in.side_rows_override = v[23];
        in.wide = v[24] != 0;
        in.wide_segments = v[25];
        check_stored_rows(in, since, T, line);
        fused_stored_rows(in, since + 2 * T * (k + 1), kind.st_lo, kind.st_hi);
        if (fused_ghosts_exhausted(in, since + 2 * T * (k + 1)) || kind.st_hi <= kind.st_lo) {
            printf("skip\n");
            continue;
        }
        const FusedPlan P = fused_plan(in, kind);
        check_plan(in, kind, P, line);
        printf("st_lo=%d st_hi=%d rows_per_chunk=%d first_rows=%d last_rows=%d n_strips=%d n_chunks=%d nb_top=%d nb_bot=%d ns_left=%d ns_right=%d "
               "side_rows=%d side_subs=%d side_rows_edge=%d first_edge=%d last_edge=%d wide_y0=%d wide_y1=%d wide_h=%d wide_nseg=%d wide_stride=%d "
               "wide_tiles=%d edge_target=%llu edge_chunks=%d edge_strips=%d n_border=%ld any_plain=%d edge=%d wide=%d wx0=%d wx1=%d n_wide=%d "
               "border_steps=%ld border_longest=%d grid_x=%u grid_y=%u bgrid_x=%u wgrid_x=%u\n",
               P.st_lo, P.st_hi, P.rows_per_chunk, P.first_rows, P.last_rows, P.n_strips, P.n_chunks, P.nb_top, P.nb_bot, P.ns_left, P.ns_right, P.side_rows,
               P.side_subs, P.side_rows_edge, P.first_edge, P.last_edge, P.wide_y0, P.wide_y1, P.wide_h, P.wide_nseg, P.wide_stride, P.wide_tiles,
               P.edge_target, P.edge_chunks, P.edge_strips, P.n_border, (int)P.any_plain, (int)P.edge, (int)P.wide, P.wx0, P.wx1, P.n_wide, P.border.steps,
               P.border.longest, P.grid_x, P.grid_y, P.bgrid_x, P.wgrid_x);
    }
    return failures ? 1 : 0;
}

static double split_cost(const FusedPassSplit &s, const double *cost)
{
    double c = 0.0;
    for (int T : s.depths) c += cost[T];
    return c;
}

static long splits()
{
    long cases = 0;
    double tables[4][kWideT + 1];
    for (int T = 0; T <= 8; ++T) {
        tables[0][T] = fused_default_cost(T);
        tables[1][T] = 0.05 + 0.11 * T;                         // a launch costs next to nothing: time goes with the depth
        tables[2][T] = T == 3 ? 0.2 : 1.0 + 0.3 * T;            // one depth far cheaper than the others
        tables[3][T] = T == 8 ? 0.9 : 1.0;                      // every depth costs about the same
    }
    for (int iterations = 2; iterations <= 130; ++iterations)
        for (int tmax = 1; tmax <= 8; ++tmax)
            for (const auto &cost : tables)
                for (int free_allowed = 0; free_allowed < 2; ++free_allowed) {
                    ++cases;
                    const FusedPassSplit s = fused_pass_split(iterations, tmax, cost, free_allowed != 0);
                    long sum = s.in_place;
                    for (size_t k = 0; k < s.depths.size(); ++k) {
                        sum += s.depths[k];
                        CHECK(s.depths[k] >= 1 && s.depths[k] <= tmax, "%d iterations, tmax %d: depth %d", iterations, tmax, s.depths[k]);
                        if (k > 0) CHECK(s.depths[k] <= s.depths[k - 1], "%d iterations, tmax %d: depths not sorted", iterations, tmax);
                    }
                    CHECK(!s.depths.empty(), "%d iterations, tmax %d: no split", iterations, tmax);
                    CHECK(sum == iterations, "%d iterations, tmax %d: the split sums to %ld", iterations, tmax, sum);
                    CHECK(s.in_place == ((tmax == 1 && (iterations & 1)) ? 1 : 0), "%d iterations, tmax %d: %d in place", iterations, tmax, s.in_place);
                    CHECK(s.free_parity == (s.depths.size() % 2 == 1), "%d iterations, tmax %d: %zu passes, free_parity %d", iterations, tmax,
                          s.depths.size(), (int)s.free_parity);
                    const FusedPassSplit even = fused_pass_split(iterations, tmax, cost, false);
                    CHECK(even.depths.size() % 2 == 0, "%d iterations, tmax %d: %zu passes without free parity", iterations, tmax, even.depths.size());
                    if (s.depths.size() % 2 == 1)
                        CHECK(free_allowed && split_cost(s, cost) < split_cost(even, cost), "%d iterations, tmax %d: an odd split that is not cheaper",
                              iterations, tmax);
                    else
                        CHECK(split_cost(s, cost) == split_cost(even, cost), "%d iterations, tmax %d: an even split that is not the best even one",
                              iterations, tmax);
                }
    // which passes store their red halves
    for (size_t n = 1; n <= 9; ++n)
        for (size_t k = 0; k < n; ++k)
            for (int l1_last = 0; l1_last < 2; ++l1_last) {
                ++cases;
                CHECK(fused_stores_red(k, n, l1_last != 0, true), "pass %zu of %zu: red_store_all", k, n);
                const bool want = k + 1 == n || (l1_last && k + 2 == n);
                CHECK(fused_stores_red(k, n, l1_last != 0, false) == want, "pass %zu of %zu, l1_last %d", k, n, l1_last);
            }
    return cases;
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "batch") == 0) return batch();
    if (argc == 2 && strcmp(argv[1], "splits") == 0) {
        const long cases = splits();
        if (failures) {
            printf("%d violations in %ld cases\n", failures, cases);
            return 1;
        }
        printf("ok %ld\n", cases);
        return 0;
    }
    if (argc >= 5 && strcmp(argv[1], "split") == 0) {
        const int iterations = atoi(argv[2]), tmax = atoi(argv[3]);
        std::vector<double> cost(tmax + 1, 0.0);
        for (int T = 1; T <= tmax; ++T) cost[T] = 4 + T < argc ? atof(argv[4 + T]) : fused_default_cost(T);
        const FusedPassSplit s = fused_pass_split(iterations, tmax, cost.data(), atoi(argv[4]) != 0);
        printf("%d %d", s.in_place, (int)s.free_parity);
        for (int T : s.depths) printf(" %d", T);
        printf("\n");
        return 0;
    }
    if (argc == 9 && strcmp(argv[1], "tune") == 0) {
        Geom g{};
        g.W = atoi(argv[2]);
        g.H = atoi(argv[3]);
        g.y0 = atoi(argv[4]);
        g.local_rows = atoi(argv[5]);
        for (int R : fused_tune_chunk_rows(g, atoi(argv[6]), atoi(argv[7]), atol(argv[8]))) printf("%d ", R);
        printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: fused_plan_check batch | splits | split ITERATIONS TMAX FREE [COSTS] | tune W H y0 local_rows C T SLOTS\n");
    return 2;
}
