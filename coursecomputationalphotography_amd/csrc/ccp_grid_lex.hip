// ccp_grid_lex.hip — the reference's own (lexicographic) sweep order on a grid handle: the ticket order, the launchers
// of the time-skewed strips and of the hyperplane engine (kernels: ccp_grid_lex.hpp), ccp_grid_gauss_seidel_lexicographic.
#include "ccp_grid_handle.hpp"
#include "ccp_grid_lex.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

using namespace ccp;

namespace {

// `iterations` lexicographic sweeps of the channels in `mask`, pipelined over the hyperplanes
// tau = x + y + 2k (ccp_grid_lex.hpp).  partial != nullptr: per-sweep step sums are written too.
// partial sums one checked sweep writes per channel
// (time-skewed strips: the strip count depends on the depth; the partial layout uses the largest, depth 8's —
// slots a shallower launch does not write must read as zero, so the buffer is cleared per batch)
// Tickets of a launch of `groups` groups of T sweeps on an image W pixels wide, in the order the strips can start: (k, s)
// follows its left neighbour (k, s-1) by a strip lag (the 62 diagonals its first pixel lies further on + the 16 steps of
// edge values it wants to see published + the publication's own lag) and the same strip of the group before by a group
// lag; a workgroup that is resident but waiting keeps a slot from one that could run.  Everything a strip waits for —
// (k, s-1), (k-1, s), the last reader of its edge buffer (k - kLexEdgeSets, s+1): lex_wg_body — holds a smaller ticket, and a
// ticket's holder never waits for a larger one: no deadlock, whatever the residency (tests/test_lex_tickets.py checks
// exactly that through ccp_debug_lex_tickets).  order[ticket] = k * strips + s, strips = lex_strip_count(W, T, groups).
void lex_ticket_order(int W, int T, int groups, std::vector<unsigned> &order)
{
    const int S = lex_strip_count(W, T, groups);
    const long strip_lag = kLexSkewCols + 34, group_lag = 19 + 4 * (T - 1) + 16;
    struct Ticket { long start; int k, s; };
    std::vector<long> start((size_t)groups * S, -1);
    std::vector<Ticket> tickets;
    for (int k = 0; k < groups; ++k)
        for (int st = lex_strip_first(T, k); st <= lex_strip_last(W, T, k); ++st) {
            long t = 0;
            if (lex_strip_exists(W, T, k, st - 1)) t = std::max(t, start[(size_t)k * S + st - 1] + strip_lag);
            if (lex_strip_exists(W, T, k - 1, st)) t = std::max(t, start[(size_t)(k - 1) * S + st] + group_lag);
            if (lex_strip_exists(W, T, k - kLexEdgeSets, st + 1)) t = std::max(t, start[(size_t)(k - kLexEdgeSets) * S + st + 1] + 1);
            start[(size_t)k * S + st] = t;
            tickets.push_back({t, k, st});
        }
    std::stable_sort(tickets.begin(), tickets.end(), [](const Ticket &a, const Ticket &b) { return a.start < b.start; });
    order.clear();
    for (const Ticket &t : tickets) order.push_back((unsigned)((long)t.k * S + t.s));
}

// the diagonal-major arrays behind their front rows (kLexFrontRows: what k_lex_wg's loader prefetches for a strip that
// starts left of the image lies up to 64 diagonals before the first one; never used)
double *lex_xd(const ccp_grid *g) { return g->lex_x.p + (size_t)kLexFrontRows * g->lexg.P; }
double *lex_bd(const ccp_grid *g) { return g->lex_b.p + (size_t)kLexFrontRows * g->lexg.P; }
constexpr int kLexBatchSweeps = 128;     // sweeps in flight between two looks at the stop rule: the first batch (later ones grow while the rule is far off)
constexpr int kLexLaunchSweeps = 1024;   // most sweeps one launch of k_lex_wg carries (its strips move 2 columns left per sweep: lex_strip_count)
long lex_partials_per_sweep(const ccp_grid *g)
{
    if (g->lex_mode == 3) return (long)lex_strip_count(g->desc.width, 1, kLexLaunchSweeps);   // (the groups of a checked batch shift by 2 x its sweeps at most)
    return (long)g->lexg.n_diag * g->lexg.nbx;
}

// `iterations` lexicographic sweeps as time-skewed strips: groups of T sweeps per pass through memory (k_lex_wg),
// T = 8, 4, 2, 1 for what is left over; every depth is one launch holding all its groups.
template <int T>
int lex_launch_skew(ccp_grid *g, int groups, unsigned mask, double *partial, int t_last = T)
{
    const LexGeom &lg = g->lexg;
    const int C = g->desc.channels;
    if ((long)groups * T > kLexLaunchSweeps) return CCP_ERR_STATE;
    const bool dbg = getenv("CCP_GS_DEBUG") != nullptr;
    const auto t_in = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (dbg) fprintf(stderr, "[ccp_gs] lex_launch_skew %s at %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count());
    };
    const int S = lex_strip_count(lg.W, T, groups);                      // strip slots per group (not every group has all of them)
    const int S_cap = lex_strip_count(lg.W, 1, kLexLaunchSweeps);       // ... of the largest launch, whatever its depth
    const long edge_steps = kWave + lg.H + 2 * (T - 1);
    // persistent workgroups: as many as are resident at once (k_lex_wg's comment), each taking strips from the ticket counter
    int per_cu = 0, cus = 0;
    if (g->masked) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_lex_wg_masked<T, false>, (T + 2) * kWave, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_lex_wg<T, false>, (T + 2) * kWave, 0);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device);
    const long resident = (long)std::max(per_cu, 1) * std::max(cus, 1);
    lap("occupancy known");
    // Buffers are sized for the largest launch a solve can issue (kLexLaunchSweeps), not for this one: a call with more
    // sweeps than the call before must not pay a 0.5 GB reallocation inside its own timing (the kernel trace of round 4
    // showed 25 ms of it between the layout conversion and the launch).
    const size_t need = (size_t)C * groups * S * kLexWordStride;
    const size_t need_cap = (size_t)C * std::max(groups, kLexLaunchSweeps / 8) * S_cap * kLexWordStride;
    const size_t edges = (size_t)kLexEdgeSets * C * S * edge_steps * 2 * T + (size_t)C * resident * kLexScratch;   // (+ the storers' scratch slots, one set per resident workgroup)
    const size_t edges_cap = (size_t)kLexEdgeSets * C * S_cap * (kWave + lg.H + 14) * 16 + (size_t)C * resident * kLexScratch;   // (what depth 8 needs)
    if (g->lex_progress.n < need) CCP_TRY(g->lex_progress.alloc(std::max(need, need_cap)));
    if (g->lex_order_groups != groups || g->lex_order_strips != S || g->lex_order_depth != T) {
        // Tickets in the order the strips can start: (k, s) follows its left neighbour (k, s-1) by a strip lag (the 62
        // diagonals its first pixel lies further on + the 16 steps of edge values it wants to see published + the
        // publication's own lag) and the same strip of the group before by a group lag; a workgroup that is resident but
        // waiting keeps a slot from one that could run.  Everything a strip waits for holds a smaller ticket — a ticket's
        // holder never waits for a larger one: no deadlock, whatever the residency.
        std::vector<unsigned> tickets;
        lex_ticket_order(lg.W, T, groups, tickets);
        if (tickets.empty()) return CCP_ERR_STATE;
        lap("tickets sorted");
        const size_t order_cap = std::max(tickets.size(), (size_t)(kLexLaunchSweeps / 8) * S_cap);
        CCP_HIP(hipStreamSynchronize(g->stream));               // (an earlier copy from the pinned buffer may still be in flight)
        lap("stream drained");
        if (g->lex_order_pin_cap < tickets.size()) {
            if (g->lex_order_pin) (void)hipHostFree(g->lex_order_pin);
            g->lex_order_pin = g->lex_order_dev = nullptr;
            g->lex_order_pin_cap = 0;
            CCP_HIP(hipHostMalloc(reinterpret_cast<void **>(&g->lex_order_pin), order_cap * sizeof(unsigned), hipHostMallocMapped));
            CCP_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&g->lex_order_dev), g->lex_order_pin, 0));
            g->lex_order_pin_cap = order_cap;
        }
        for (size_t i = 0; i < tickets.size(); ++i) g->lex_order_pin[i] = tickets[i];
        __atomic_thread_fence(__ATOMIC_RELEASE);
        g->lex_order_count = tickets.size();
        g->lex_order_groups = groups;
        g->lex_order_strips = S;
        g->lex_order_depth = T;
        lap("order queued");
    }
    const unsigned n_tickets = (unsigned)g->lex_order_count;
    const long wgs = std::max<long>(1, std::min<long>((long)n_tickets, (resident + C - 1) / C));
    if (g->lex_edges.n < edges) CCP_TRY(g->lex_edges.alloc(std::max(edges, edges_cap)));
    if (!g->lex_ticket.p) CCP_TRY(g->lex_ticket.alloc(kMaxChannels));
    CCP_HIP(hipMemsetAsync(g->lex_progress.p, 0, need * sizeof(unsigned), g->stream));
    CCP_HIP(hipMemsetAsync(g->lex_ticket.p, 0, kMaxChannels * sizeof(unsigned), g->stream));
    dim3 grid((unsigned)wgs, (unsigned)C);
    lap("buffers cleared");
    if (getenv("CCP_GS_DEBUG"))
        fprintf(stderr, "[ccp_gs] k_lex_wg<%d>: %d workgroups per CU on %d CUs, %ld persistent workgroups per channel for %d groups x %d strips\n",
                T, per_cu, cus, wgs, groups, S);
    const dim3 block((T + 2) * kWave);
    double *nop = nullptr;
    unsigned long long *trace = nullptr;
    const size_t trace_words = (size_t)4 * C * groups * S;
    if (g->trace_file) {
        if (g->trace.n < trace_words) CCP_TRY(g->trace.alloc(trace_words));
        CCP_HIP(hipMemsetAsync(g->trace.p, 0, trace_words * sizeof(unsigned long long), g->stream));
        trace = g->trace.p;
    }
#define CCP_LEX_WG(KERNEL, CHECK, P, STRIDE)                                                                                        \
    hipLaunchKernelGGL((KERNEL<T, CHECK>), grid, block, 0, g->stream,                                                                \
                       LexWgArgs{lex_xd(g), lex_bd(g), g->geom, lg, groups, S, n_tickets, g->lex_progress.p, g->lex_ticket.p, g->lex_order_dev,  \
                                 g->lex_edges.p, edge_steps, mask, P, STRIDE, trace, t_last})
    if (g->masked) {
        if (partial) CCP_LEX_WG(k_lex_wg_masked, true, partial, lex_partials_per_sweep(g));
        else CCP_LEX_WG(k_lex_wg_masked, false, nop, 0L);
    } else {
        if (partial) CCP_LEX_WG(k_lex_wg, true, partial, lex_partials_per_sweep(g));
        else CCP_LEX_WG(k_lex_wg, false, nop, 0L);
    }
#undef CCP_LEX_WG
    CCP_HIP(hipGetLastError());
    if (trace) {
        CCP_HIP(hipStreamSynchronize(g->stream));
        std::vector<unsigned long long> host(trace_words);
        CCP_HIP(hipMemcpy(host.data(), trace, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *f = fopen(g->trace_file, "ab")) {
            // (the same 8-word header as the fused passes' records, tag "LEXTRAC")
            const unsigned long long head[8] = {0x4341525458454cull, (unsigned long long)T, (unsigned long long)groups, (unsigned long long)S,
                                                (unsigned long long)C, (unsigned long long)lg.H, (unsigned long long)host.size(), (unsigned long long)lg.W};
            fwrite(head, sizeof(head), 1, f);
            fwrite(host.data(), sizeof(unsigned long long), host.size(), f);
            fclose(f);
        }
    }
    return CCP_OK;
}

int lex_run_skew(ccp_grid *g, int iterations, unsigned mask, double *partial)
{
    const int C = g->desc.channels;
    const long per_sweep = (long)C * lex_partials_per_sweep(g);          // partial doubles per sweep (all channels)
    int left = iterations, done = 0;
    if (g->lex_tmax >= 8 && left >= 8 && left % 8 != 0) {
        // a count that is not a multiple of 8: ONE launch of depth-8 groups whose last group passes the sweeps it does
        // not have through (lex_wg_pass_through) instead of remainder launches of depth 4, 2, 1, each a pipeline of its
        // own to fill and drain.  (With the stop rule too: the passed-through sweeps leave step sums of 0 in slots
        // beyond the batch's last sweep, which nobody reads; the partial buffer holds whole groups.)
        const int groups = (left + 7) / 8;
        return lex_launch_skew<8>(g, groups, mask, partial, left - 8 * (groups - 1));
    }
    for (int T = 8; T >= 1; T >>= 1) {
        if (T > g->lex_tmax || left < T) continue;
        const int groups = left / T;
        double *p = partial ? partial + (long)done * per_sweep : nullptr;
        if (T == 8) CCP_TRY(lex_launch_skew<8>(g, groups, mask, p));
        else if (T == 4) CCP_TRY(lex_launch_skew<4>(g, groups, mask, p));
        else if (T == 2) CCP_TRY(lex_launch_skew<2>(g, groups, mask, p));
        else CCP_TRY(lex_launch_skew<1>(g, groups, mask, p));
        done += groups * T;
        left -= groups * T;
    }
    return CCP_OK;
}

int lex_run(ccp_grid *g, int iterations, unsigned mask, double *partial)
{
    if (g->lex_mode == 3 && iterations > 0) return lex_run_skew(g, iterations, mask, partial);
    const LexGeom &lg = g->lexg;
    const int d_max = lg.n_diag - 1;
    const int C = g->desc.channels;
    for (int tau = 0; tau <= d_max + 2 * (iterations - 1); ++tau) {
        const int k_lo = std::max(0, (tau - d_max + 1) / 2);          // smallest k with tau - 2k <= d_max
        const int k_hi = std::min(iterations - 1, tau / 2);           // largest k with tau - 2k >= 0
        if (k_hi < k_lo) continue;
        dim3 grid((unsigned)lg.nbx, (unsigned)(k_hi - k_lo + 1), (unsigned)C);
        if (partial)
            hipLaunchKernelGGL((k_lex_plane<true>), grid, dim3(kBlock), 0, g->stream, lex_xd(g), lex_bd(g), g->geom, lg,
                               tau, k_lo, mask, partial);
        else
            hipLaunchKernelGGL((k_lex_plane<false>), grid, dim3(kBlock), 0, g->stream, lex_xd(g), lex_bd(g), g->geom, lg,
                               tau, k_lo, mask, static_cast<double *>(nullptr));
    }
    CCP_HIP(hipGetLastError());
    return CCP_OK;
}

}  // namespace

extern "C" {

int ccp_grid_gauss_seidel_lexicographic(ccp_grid *g, double epsilon, int32_t max_iteration, int32_t check_every,
                                        ccp_gs_report *report)
try {
    CCP_TRY(not_weighted(g));
    CCP_TRY(bind(g));
    if (g->ghost_top || g->ghost_bottom || g->desc.row_count != g->desc.height) return CCP_ERR_STATE;   // whole image only
    if (g->masked && g->lex_mode != 3) return CCP_ERR_UNSUPPORTED;  // Dirichlet masks: k_lex_wg only
    if (max_iteration < 0 || check_every < 0) return CCP_ERR_BAD_ARG;
    const int C = g->desc.channels, W = g->desc.width, H = g->desc.height;
    LexGeom &lg = g->lexg;
    lg.W = W;
    lg.H = H;
    lg.P = ((long)W + 15) / 16 * 16;
    lg.n_diag = W + H - 1;
    lg.plane = (long)lg.n_diag * lg.P;
    lg.nbx = (std::min(W, H) + kLexTile - 1) / kLexTile;
    const size_t elems = (size_t)lg.plane * C;
    const size_t slack = (size_t)kLexSlackRows * lg.P;       // k_lex_wg prefetches some diagonals past the last one (never used)
    const size_t front = (size_t)kLexFrontRows * lg.P;       // ... and a strip that starts left of the image some diagonals before the first
    if (g->lex_x.n != front + elems + slack) {
        CCP_TRY(g->lex_x.alloc(front + elems + slack));
        CCP_TRY(g->lex_b.alloc(front + elems + slack));
        CCP_HIP(hipMemsetAsync(g->lex_x.p, 0, front * sizeof(double), g->stream));
        CCP_HIP(hipMemsetAsync(g->lex_b.p, 0, front * sizeof(double), g->stream));
        CCP_HIP(hipMemsetAsync(lex_xd(g) + elems, 0, slack * sizeof(double), g->stream));
        CCP_HIP(hipMemsetAsync(lex_bd(g) + elems, 0, slack * sizeof(double), g->stream));
    }
    CCP_TRY(begin_timing(g));
    dim3 cgrid((unsigned)((W + kBlock - 1) / kBlock), (unsigned)H, (unsigned)C);
    dim3 tgrid((unsigned)((W + kLexCT - 1) / kLexCT), (unsigned)((H + kLexCT - 1) / kLexCT), (unsigned)C);
    dim3 sgrid((unsigned)((W + kLexCT - 1) / kLexCT), (unsigned)((lg.n_diag + kLexCT - 1) / kLexCT), (unsigned)C);
    hipLaunchKernelGGL(k_lex_to_diag_sheared, sgrid, dim3(kBlock), 0, g->stream, g->x.p, lex_xd(g), g->geom, lg);
    if (g->masked) hipLaunchKernelGGL(k_lex_convert_b_masked, cgrid, dim3(kBlock), 0, g->stream, g->b.p, g->maskp.p, lex_bd(g), g->geom, lg);
    else hipLaunchKernelGGL(k_lex_to_diag_sheared, sgrid, dim3(kBlock), 0, g->stream, g->b.p, lex_bd(g), g->geom, lg);
    CCP_HIP(hipGetLastError());

    const unsigned all = (C >= 32) ? 0xffffffffu : ((1u << C) - 1u);
    int iterations_of[kMaxChannels], converged[kMaxChannels];
    double last_eps[kMaxChannels];
    for (int ch = 0; ch < C; ++ch) {
        iterations_of[ch] = max_iteration;
        converged[ch] = 0;
        last_eps[ch] = 10.0;                                              // `double eps = 10` (sparse-matrix.h:354)
    }
    if (check_every == 0 || !(10.0 > epsilon)) {
        // fixed count — or the reference loop never starts (eps = 10 <= epsilon)
        const int n = check_every == 0 ? max_iteration : 0;
        for (int done = 0; done < n;) {                    // gridDim.y carries the sweeps in flight: keep it small
            const int kb = std::min(g->lex_mode != 0 ? kLexLaunchSweeps : 32768, n - done);   // (k_lex_wg: one progress word per group and strip)
            CCP_TRY(lex_run(g, kb, all, nullptr));
            done += kb;
        }
        for (int ch = 0; ch < C; ++ch) iterations_of[ch] = n;
    } else {
        // Sweeps in flight between two looks at the rule: kLexBatchSweeps to begin with, doubled (up to one launch's worth)
        // while every channel's step, at the rate it has been shrinking, is more than four batches away from epsilon.  A
        // batch is one pipeline to fill and drain and one snapshot; a channel that stops inside a batch is redone from the
        // snapshot for exactly the sweeps the reference would have made — the result does not depend on the batching.  (The
        // reference's defaults, epsilon 1e-6 and 1,000 sweeps, never stop early on an image-sized system: 8 batches of 128
        // were 7.0 ms at 512^2 where one pipeline of 1,000 sweeps is 2.5 ms.)
        const int batch_cap = g->lex_mode == 3 ? kLexLaunchSweeps : kLexBatchSweeps;
        int batch = kLexBatchSweeps;
        const long per = lex_partials_per_sweep(g);                         // partials per (iteration, channel)
        if (g->lex_partial.n != (size_t)per * batch_cap * C) CCP_TRY(g->lex_partial.alloc((size_t)per * batch_cap * C));
        if (g->lex_eps.n != (size_t)batch_cap * C) CCP_TRY(g->lex_eps.alloc((size_t)batch_cap * C));
        if (g->lex_snap.n != elems) CCP_TRY(g->lex_snap.alloc(elems));
        std::vector<double> eps_vec((size_t)batch_cap * C);
        double *eps_host = eps_vec.data();
        unsigned mask = all;
        int done = 0;
        while (mask && done < max_iteration) {
            const int kb = std::min(batch, max_iteration - done);
            CCP_HIP(hipMemcpyAsync(g->lex_snap.p, lex_xd(g), elems * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
            if (g->lex_mode == 3) CCP_HIP(hipMemsetAsync(g->lex_partial.p, 0, sizeof(double) * (size_t)per * kb * C, g->stream));
            CCP_TRY(lex_run(g, kb, mask, g->lex_partial.p));
            hipLaunchKernelGGL(k_lex_reduce, dim3((unsigned)kb, (unsigned)C), dim3(kBlock), 0, g->stream, g->lex_partial.p, per,
                               g->lex_eps.p);
            CCP_HIP(hipGetLastError());
            CCP_HIP(hipMemcpyAsync(eps_host, g->lex_eps.p, sizeof(double) * kb * C, hipMemcpyDeviceToHost, g->stream));
            CCP_HIP(hipStreamSynchronize(g->stream));
            // how far the rule is, in sweeps, for the channel nearest to it (the step of the batch's last sweep against
            // the one half a batch earlier)
            double nearest = 1e300;
            for (int ch = 0; ch < C && kb >= 2; ++ch) {
                if (!((mask >> ch) & 1u)) continue;
                const double e1 = eps_host[(size_t)(kb - 1) * C + ch], e0 = eps_host[(size_t)(kb / 2 - 1) * C + ch];
                double left = 1e300;
                if (!(e1 > epsilon)) left = 0.0;
                else if (e1 < e0 && epsilon > 0.0) left = std::log(epsilon / e1) / (std::log(e1 / e0) / (double)(kb - kb / 2));
                nearest = std::min(nearest, left);
            }
            if (nearest > 4.0 * batch) batch = std::min(batch * 2, batch_cap);
            for (int ch = 0; ch < C; ++ch) {
                if (!((mask >> ch) & 1u)) continue;
                int stop = -1;
                for (int k = 0; k < kb; ++k) {
                    if ((done + k + 1) % check_every != 0) continue;
                    last_eps[ch] = eps_host[(size_t)k * C + ch];
                    if (!(last_eps[ch] > epsilon)) {
                        stop = k;
                        break;
                    }
                }
                if (stop < 0) continue;
                converged[ch] = 1;
                iterations_of[ch] = done + stop + 1;
                mask &= ~(1u << ch);
                if (stop < kb - 1) {
                    // the pipeline ran past the sweep the rule stops at: redo exactly stop+1 sweeps of
                    // this channel from the snapshot taken before the batch
                    CCP_HIP(hipMemcpyAsync(lex_xd(g) + (size_t)ch * lg.plane, g->lex_snap.p + (size_t)ch * lg.plane,
                                           (size_t)lg.plane * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
                    CCP_TRY(lex_run(g, stop + 1, 1u << ch, nullptr));
                }
            }
            done += kb;
        }
        for (int ch = 0; ch < C; ++ch)
            if (!converged[ch]) iterations_of[ch] = done;
    }
    hipLaunchKernelGGL((k_lex_convert_tiled<false>), tgrid, dim3(kBlock), 0, g->stream, g->x.p, lex_xd(g), g->geom, lg);
    CCP_HIP(hipGetLastError());
    return finish_solve(g, report, [&](int ch, ccp_gs_report &r) {
        r.converged = converged[ch];
        r.iterations = iterations_of[ch];
        r.last_l1_step = last_eps[ch];
    });
} CCP_ABI_CATCH

int ccp_debug_lex_tickets(int32_t width, int32_t depth, int32_t groups, uint32_t *order, int64_t capacity, int32_t *strips, int64_t *count)
try {
    if (width < 1 || groups < 1 || (depth != 1 && depth != 2 && depth != 4 && depth != 8) || (long)groups * depth > kLexLaunchSweeps || !strips || !count)
        return CCP_ERR_BAD_ARG;
    std::vector<unsigned> t;
    lex_ticket_order(width, depth, groups, t);
    *strips = lex_strip_count(width, depth, groups);
    *count = (int64_t)t.size();
    if (order) {
        if (capacity < (int64_t)t.size()) return CCP_ERR_BAD_ARG;
        std::copy(t.begin(), t.end(), order);
    }
    return CCP_OK;
} CCP_ABI_CATCH

}  // extern "C"
