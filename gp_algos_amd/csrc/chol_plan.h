// The single-launch Cholesky's planner: the task list chol_mega_kernel (kernels_diag.hip) works through, its list schedule and the
// replay that checks a list.  Host C++ over standard headers only -- no HIP, no gpcore_internal.h -- so that it also builds into a
// stand-alone program with the host compiler and its sanitizers (tests/chol_plan_main.cpp).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

constexpr int CHOL_PLAN_NB = 128;   // the block edge, GP_NB of gpcore_internal.h (asserted equal in gpcore_chol.hip)

struct mega_task { int type, k0, kb, i, j, q, dep[10]; };
static_assert(sizeof(mega_task) == 16 * sizeof(int), "chol_mega_kernel reads 16 ints per task (gpk_chol_mega)");
struct mega_plan { int np = 0, extra = 0, out_blocks = 0, workers = 0; double model_us = 0.0; std::vector<mega_task> tasks; };

// ---- the factorisation of ONE matrix as one persistent launch (chol_mega_kernel, kernels_diag.hip) ----
// Task list of the two-level right-looking factorisation (inner 128, outer panels of `out_blocks` block columns), in a LIST-SCHEDULE
// order: the tasks are generated in the order chol_blocked launches them, a critical-path-first schedule of that DAG on `workers`
// workgroups is simulated with a cost model (us per task on one CU, measured with tools/mega_trace.py: the constants below; a hand-over
// between workgroups 3), and the list is the tasks in the order the simulation starts them.  Workgroups claim tasks in list order, so
// on the chip the dependencies of a claimed task are mostly met already.  Every dependency points BACKWARDS in the list (checked):
// no deadlock.  The model is accurate -- with the measured task costs its makespan at n = 8192 is 4.79 ms against 4.7-4.85 measured --
// so it also answers what-ifs without a GPU (gp_chol_plan_info with GPCORE_MEGA_COSTS): K = 512 tile at 65 instead of 77.7 us 4.33 ms,
// the link at half its time 4.71 ms, tiles for free 3.86 ms.
// What the static order leaves on the table, and what did not recover it (round 4; the traces are tools/mega_trace.py's, the scheduling
// variants are kept as tools/lab/mega_claim_ahead.patch):
//   - the mean step from one diagonal block to the next is ~75 us against ~57 of task bodies: in some phases of the factorisation the
//     chip is behind the model and the chain's tasks are claimed 10-60 us after their dependencies were met, in others it is ahead and
//     they are claimed up to 400 us early (profiles/r04_i_mega_chain_detail.log);
//   - the chain's tasks a fixed lead (0..200 us of model time) earlier in the list: 4.99-5.09 ms, the lag is not a constant
//     (profiles/r04_k_fit_mega_lead_sweep.log);
//   - the chain's tasks in a queue of their own whose head is taken, by compare-and-swap, by the first workgroup that finds it READY:
//     nobody spins, but the head moves one task per poll of one workgroup (~2 us) and the 33 quarters behind a panel boundary are taken
//     over 66 us: 5.63 ms (profiles/r04_j_*);
//   - that queue claimed a bounded number of tasks AHEAD (4..64 outstanding) by workgroups that then wait: 5.27-6.03 ms, every
//     outstanding task is a CU spinning and the late dependencies are one level further out, in the bulk (profiles/r04_l_*, r04_m_*:
//     with every in-panel task of the next 2 / 4 / 8 block rows in the chain queue 5.47 / 5.53 / 5.65 ms);
//   - every block's link given an early phase INSIDE its task (the previous panel's earlier block columns applied before block k-1's
//     factor arrives): 4.92-5.10 ms, no better (profiles/r04_i_fit_mega_lead_order.log).  What is kept instead is that early part as
//     tasks of their own (type 5, below): the gap across a panel boundary fell from 85 to 15 us, the gaps inside panels rose from 8 to
//     18 us, the mean step stayed -- 2-7 % at n = 5120 ... 14336 (profiles/r04_q_*);
//   - pairs of tiles as 256 x 128 tasks: in the model 5.35 ms at n = 8192 (coarser tasks stand in the chain's way), 4.69 when only
//     columns a panel or more to the right are paired; not built.
inline bool chol_mega_plan(int np, int extra, int out_blocks, int workers, mega_plan &plan) {
    const int nb = np / CHOL_PLAN_NB, nrow = (np + extra) / CHOL_PLAN_NB;
    struct node { mega_task t; double cost; std::vector<int> deps; };
    std::vector<node> g;
    g.reserve((size_t)nb * nb);
    std::vector<int> trsm_of((size_t)nb * nrow, -1), potrf_of(nb, -1);
    // last writers of a tile: the task(s) whose result the next reader / writer of tile (i, j) must wait for (up to 4 quarters)
    std::vector<std::vector<int>> last((size_t)nrow * nb);
    auto tile = [&](int i, int j) -> std::vector<int> & { return last[(size_t)i * nb + j]; };
    // us per task on one CU, from tools/mega_trace.py (profiles/r04_q_mega_trace_boundary_sums.log): body + publish
    // (the list is not sensitive to them: with every cost 10 % lower or higher, or the link at 45 instead of 30, n = 8192 refits in
    // 4.80-4.90 ms, profiles/r04_r_fit_mega_cost_model_sweep.log)
    double c_potrf = 27.5, c_trsm = 20.8, c_k128 = 25.1, c_k512 = 77.7, c_q128 = 9.0, c_q512 = 27.8, c_link = 30.0;
    if (const char *e = getenv("GPCORE_MEGA_COSTS"))      // lab: "potrf,trsm,k128,k512,q128,q512,link" -- what-if runs of the model (gp_chol_plan_info)
        sscanf(e, "%lf,%lf,%lf,%lf,%lf,%lf,%lf", &c_potrf, &c_trsm, &c_k128, &c_k512, &c_q128, &c_q512, &c_link);
    auto add = [&](int type, int k0, int kb, int i, int j, int q, double cost, std::vector<int> deps) {
        node nd;
        nd.t = mega_task{type, k0, kb, i, j, q, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};
        nd.cost = cost;
        std::sort(deps.begin(), deps.end());
        deps.erase(std::unique(deps.begin(), deps.end()), deps.end());
        nd.deps = deps;
        g.push_back(nd);
        return (int)g.size() - 1;
    };
    std::vector<int> pre_x;       // writers of tile (k+1, k) before its rows are solved: what the fused task of block k+1 waits for
    std::vector<int> early;       // the type-5 quarters of the next panel's first diagonal tile
    for (int c0 = 0; c0 < nb; c0 += out_blocks) {
        const int c1 = std::min(nb, c0 + out_blocks);
        for (int k = c0; k < c1; ++k) {
            if (k == 0) potrf_of[k] = add(0, k, 1, k, k, -1, c_potrf, tile(k, k));
            else {
                // every later block: the link to block k-1 (solve of rows k of block column k-1, the update of tile (k, k) that those rows
                // complete) is the prologue of the diagonal block's task; the place holder made in step k-1 stands for the solved rows.
                // Inside a panel that update is the in-panel one (K = 128, summed from zero).  For a panel's FIRST block it is the previous
                // panel's outer update of the tile: its earlier block columns were summed ahead of time by the type-5 quarters made in
                // step k-2 (slot = the panel's number), the task continues that sum (field j = the slot).
                std::vector<int> d = tile(k, k);
                d.insert(d.end(), pre_x.begin(), pre_x.end());
                d.push_back(potrf_of[k - 1]);
                int slot = -1;
                if (k == c0 && !early.empty()) { slot = c0 / out_blocks; d.insert(d.end(), early.begin(), early.end()); early.clear(); }
                potrf_of[k] = add(4, k, 1, k, slot, trsm_of[(size_t)(k - 1) * nrow + k], c_link + c_potrf, d);
                g[trsm_of[(size_t)(k - 1) * nrow + k]].t.kb = potrf_of[k];      // the place holder remembers who announces it
            }
            tile(k, k) = {potrf_of[k]};
            for (int i = k + 1; i < nrow; ++i) {
                if (i == k + 1 && i < nb) {
                    pre_x = tile(i, k);
                    trsm_of[(size_t)k * nrow + i] = add(3, k, -1, i, k, -1, -1.0, {});
                    tile(i, k) = {trsm_of[(size_t)k * nrow + i]};
                    continue;
                }
                std::vector<int> d = tile(i, k);
                d.push_back(potrf_of[k]);
                trsm_of[(size_t)k * nrow + i] = add(1, k, 1, i, k, -1, c_trsm, d);
                tile(i, k) = {trsm_of[(size_t)k * nrow + i]};
            }
            if (k == c1 - 2 && c1 < nb) {
                // the next panel's first diagonal tile: all but the last block column of ITS outer update can be summed now (rows c1 of
                // the block columns c0 .. c1-2 are solved), into the panel's scratch tile -- three quarters, (0, 1) is above the diagonal
                const int kb = c1 - 1 - c0;
                std::vector<int> d;
                for (int kk = c0; kk <= k; ++kk) d.push_back(trsm_of[(size_t)kk * nrow + c1]);
                for (int q = 0; q < 4; ++q)
                    if (q != 2) early.push_back(add(5, c0, kb, c1, c1 / out_blocks, q, c_q128 + (c_q512 - c_q128) * (kb - 1) / 3.0, d));
            }
            for (int j = k + 1; j < c1; ++j)
                for (int i = j; i < nrow; ++i) {
                    if (i == k + 1 && j == k + 1) continue;      // the next diagonal tile's update is part of that block's fused task
                    std::vector<int> d = tile(i, j);
                    d.push_back(trsm_of[(size_t)k * nrow + i]);
                    d.push_back(trsm_of[(size_t)k * nrow + j]);
                    tile(i, j) = {add(2, k, 1, i, j, -1, c_k128, d)};
                }
        }
        for (int j = c1; j < nb; ++j)
            for (int i = j; i < nrow; ++i) {
                std::vector<int> d = tile(i, j);
                d.push_back(trsm_of[(size_t)(c1 - 1) * nrow + i]);      // block column c1-1 of row block i is the last of the panel to be solved
                d.push_back(trsm_of[(size_t)(c1 - 1) * nrow + j]);
                const int kb = c1 - c0;
                const double cost = c_k128 + (c_k512 - c_k128) * (kb - 1) / 3.0, qcost = c_q128 + (c_q512 - c_q128) * (kb - 1) / 3.0;
                if (i == c1 && j == c1) continue;      // the next panel's first diagonal tile: type-5 quarters + that block's fused task
                if (i < c1 + out_blocks && j < c1 + out_blocks && i < nb) {      // the next outer panel's diagonal block: quarters
                    std::vector<int> w;
                    for (int q = 0; q < 4; ++q)
                        if (!(i == j && q == 2)) w.push_back(add(2, c0, kb, i, j, q, qcost, d));   // q = (row half) + 2 (column half); (0, 1) is above the diagonal
                    tile(i, j) = w;
                } else tile(i, j) = {add(2, c0, kb, i, j, -1, cost, d)};
            }
    }
    const int n = (int)g.size();
    for (const node &nd : g) if (nd.deps.size() > 10) return false;
    // critical-path priorities and the simulated list schedule
    const double hop = 3.0;
    std::vector<std::vector<int>> succ(n);
    std::vector<int> indeg(n, 0);
    for (int t = 0; t < n; ++t) { indeg[t] = (int)g[t].deps.size(); for (int d : g[t].deps) succ[d].push_back(t); }
    std::vector<double> prio(n, 0.0), est(n, 0.0), start(n, 0.0);
    for (int pass = 0; pass < 2; ++pass)      // twice: a fused task inherits the urgency of what waits for the rows it announces half-way
        for (int t = n - 1; t >= 0; --t) {
            double m = 0.0;
            for (int s2 : succ[t]) m = std::max(m, prio[s2]);
            prio[t] = std::max(g[t].cost, 0.0) + hop + m;
            if (g[t].t.type == 4) prio[t] = std::max(prio[t], c_link + hop + prio[g[t].t.q]);
        }
    typedef std::pair<double, int> pdi;
    std::priority_queue<pdi> ready;                                               // (priority, task): dependencies done
    std::priority_queue<pdi, std::vector<pdi>, std::greater<pdi>> waiting;        // (earliest start, task): done, but the hand-over is still in flight
    std::priority_queue<pdi, std::vector<pdi>, std::greater<pdi>> running;        // (finish time, task)
    for (int t = 0; t < n; ++t) if (indeg[t] == 0 && g[t].t.type != 3) ready.push(pdi(prio[t], t));
    int freew = workers, finished = 0;
    double now = 0.0;
    while (finished < n) {
        while (!waiting.empty() && waiting.top().first <= now + 1e-9) { const int t = waiting.top().second; waiting.pop(); ready.push(pdi(prio[t], t)); }
        while (freew > 0 && !ready.empty()) {
            const int t = ready.top().second;
            ready.pop();
            start[t] = now;
            running.push(pdi(now + g[t].cost, t));
            --freew;
            if (g[t].t.type == 4) {      // its place holder: announced c_link into the task, costs nobody a workgroup
                const int ph = g[t].t.q;
                start[ph] = now + 1e-3;
                running.push(pdi(now + c_link, ph));
            }
        }
        double next = running.empty() ? 1e300 : running.top().first;
        if (freew > 0 && !waiting.empty()) next = std::min(next, waiting.top().first);
        if (next >= 1e300) return false;      // not reached for a valid DAG
        now = next;
        while (!running.empty() && running.top().first <= now + 1e-9) {
            const int t = running.top().second;
            running.pop();
            ++finished;
            if (g[t].t.type != 3) ++freew;
            for (int s2 : succ[t]) {
                est[s2] = std::max(est[s2], now + hop);
                if (--indeg[s2] == 0) waiting.push(pdi(est[s2], s2));
            }
        }
    }
    std::vector<int> order(n), pos(n);
    for (int t = 0; t < n; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return start[a] < start[b] || (start[a] == start[b] && prio[a] > prio[b]); });
    for (int p2 = 0; p2 < n; ++p2) pos[order[p2]] = p2;
    plan.tasks.resize(n);
    for (int p2 = 0; p2 < n; ++p2) {
        const node &nd = g[order[p2]];
        mega_task t = nd.t;
        for (size_t d = 0; d < nd.deps.size(); ++d) {
            t.dep[d] = pos[nd.deps[d]];
            if (t.dep[d] >= p2) return false;      // a dependency that does not point backwards: never for a schedule (a task starts after its dependencies end)
        }
        if (t.type == 4) t.q = pos[t.q];           // the place holder it announces, by its place in the list
        if (t.type == 3) t.kb = pos[t.kb];
        plan.tasks[p2] = t;
    }
    plan.np = np, plan.extra = extra, plan.out_blocks = out_blocks, plan.workers = workers, plan.model_us = now;
    return true;
}

// independent check of the list a plan of the n x n matrix (+ extra_rows) holds: replay it and count, per tile, the updates in the order the
// two-level scheme applies them
inline bool chol_mega_plan_check(const mega_plan &pl, int n, int extra_rows) {
    const int ob = pl.out_blocks;
    const int nb = n / CHOL_PLAN_NB, nrow = (n + extra_rows) / CHOL_PLAN_NB;
    std::vector<int> upd((size_t)nrow * nb, 0), quarters((size_t)nrow * nb, 0), solved((size_t)nrow * nb, 0), fact(nb, 0), started(nb, 0);
    auto expected = [&](int i, int j) { const int J = j / ob; return J + (j - J * ob); };      // outer updates of the panels before j's, then the in-panel ones
    for (size_t p2 = 0; p2 < pl.tasks.size(); ++p2) {
        const mega_task &t = pl.tasks[p2];
        for (int d = 0; d < 10; ++d) if (t.dep[d] >= (int)p2) return false;
        if (t.type == 3) continue;                       // a place holder: announced by the fused task that names it
        if (t.type == 0) { if (upd[(size_t)t.k0 * nb + t.k0] != expected(t.k0, t.k0) || fact[t.k0]++) return false; }
        else if (t.type == 5) {
            // a quarter of the started sum of a panel's first diagonal tile: rows t.i of the previous panel's block columns but the last,
            // all solved; three quarters per slot, each once
            const int k = t.i;
            if (k % ob != 0 || k == 0 || t.j != k / ob || t.k0 != k - ob || t.kb != ob - 1 || t.q < 0 || t.q > 3 || t.q == 2 || fact[k]) return false;
            for (int kk = t.k0; kk < t.k0 + t.kb; ++kk) if (!solved[(size_t)k * nb + kk]) return false;
            if (started[k] & (1 << t.q)) return false;
            started[k] |= 1 << t.q;
        }
        else if (t.type == 4) {
            // link + diagonal block: solves rows k of block column k-1 (after all ITS updates) and completes the update of tile (k, k) those
            // rows belong to: the in-panel one, or -- first block of a panel -- the previous panel's outer one, continued from its slot
            const int k = t.k0;
            if (k == 0 || !fact[k - 1] || upd[(size_t)k * nb + (k - 1)] != expected(k, k - 1) || solved[(size_t)k * nb + (k - 1)]++) return false;
            if (k % ob == 0 && ob > 1 ? (t.j != k / ob || started[k] != 0xB) : (t.j != -1)) return false;
            if (t.q < 0 || t.q >= (int)pl.tasks.size() || pl.tasks[t.q].type != 3 || (size_t)t.q <= p2) return false;   // its place holder follows it in the list
            if (++upd[(size_t)k * nb + k] != expected(k, k) || fact[k]++) return false;
        }
        else if (t.type == 1) { if (!fact[t.k0] || upd[(size_t)t.i * nb + t.k0] != expected(t.i, t.k0) || solved[(size_t)t.i * nb + t.k0]++) return false; }
        else {
            for (int kk = t.k0; kk < t.k0 + t.kb; ++kk) if (!solved[(size_t)t.i * nb + kk] || (t.j < nb && t.i != t.j && !solved[(size_t)t.j * nb + kk])) return false;
            int &qd = quarters[(size_t)t.i * nb + t.j];
            const int need = t.q < 0 ? 1 : (t.i == t.j ? 3 : 4);
            if (++qd == need) { qd = 0; ++upd[(size_t)t.i * nb + t.j]; }
        }
    }
    for (int k = 0; k < nb; ++k) if (!fact[k]) return false;
    for (int j = 0; j < nb; ++j) for (int i = j + 1; i < nrow; ++i) if (!solved[(size_t)i * nb + j]) return false;
    return true;
}
