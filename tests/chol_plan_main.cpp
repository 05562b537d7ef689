// Stand-alone driver of the single-launch Cholesky's planner (gp_algos_amd/csrc/chol_plan.h) for a host build under
// -fsanitize=address,undefined (tests/test_chol_plan_cpu.py): plans and replays the shapes below, exits 0 when every plan is a
// valid schedule.
#include "chol_plan.h"

int main() {
    const int out_blocks = 512 / CHOL_PLAN_NB;      // the library's outer panel (GP_OUTER) in blocks
    int bad = 0, plans = 0;
    auto run = [&](int nb, int extra, int workers) {
        mega_plan pl;
        const int n = nb * CHOL_PLAN_NB;
        const bool ok = chol_mega_plan(n, extra, out_blocks, workers, pl) && chol_mega_plan_check(pl, n, extra) && !pl.tasks.empty() && pl.model_us > 0.0;
        if (!ok) { std::fprintf(stderr, "chol_plan: nb = %d extra = %d workers = %d: no valid plan\n", nb, extra, workers); ++bad; }
        ++plans;
    };
    std::vector<int> sizes;
    for (int nb = 1; nb <= 41; ++nb) sizes.push_back(nb);
    sizes.push_back(64);
    sizes.push_back(112);
    for (int nb : sizes)
        for (int extra : {0, CHOL_PLAN_NB}) {
            run(nb, extra, 256);
            if (nb == 5 || nb == 17 || nb == 41) run(nb, extra, 3);
        }
    std::printf("chol_plan: %d plans, %d bad\n", plans, bad);
    return bad ? 1 : 0;
}
