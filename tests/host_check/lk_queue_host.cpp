// lk_queue_host.cpp -- TEST ONLY.  The draw / steal rule and the work-item numbering of vo_lkqueue.h (lk_queue_take,
// lk_block_item, lk_queue_grid: the text lk_circular_queue_kernel runs) under a host simulation of workgroup arrival orders, as a
// g++ program (built with -fsanitize=address,undefined by tests/test_lk_queue_on_host.py).
//     lk_queue_host      prints "OK <geometries> <arrival orders>", exit 0; a broken rule: the case, exit 1
// A workgroup is a call of lk_queue_take with draw = fetch-and-add on the simulated counters.  Orders: dispatch order, reverse,
// one XCD entirely first, and 200 seeded random interleavings -- there a workgroup's draws are interleaved with other
// workgroups': before any of its draws, whole other workgroups (picked at random, nested up to three deep) may run.
// Checked per order: every (ticket, queue) item is taken exactly once and nothing else is; the items map one to one onto
// (frame, feature) of every frame slot of the groups; no workgroup draws more than 8 times; every surplus workgroup ends, and as
// many workgroups end without an item as the grid has surplus.
#include "../../visual_odom_amd/csrc/vo_lkqueue.h"

#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

using namespace vo;

struct Sim {
    LkQueueGrid g;
    unsigned ctr[LKQ_QUEUES] = {};
    std::vector<int> taken;     // per work item: how often it was handed out
    std::vector<char> started;  // per workgroup
    std::vector<int> pending;   // workgroups not yet started, for the nested interleavings
    std::mt19937 *rng = nullptr;
    int none = 0, most_draws = 0, marks = 0, depth = 0;
    bool bad = false;

    explicit Sim(const LkQueueGrid &grid) : g(grid), taken((size_t)LKQ_QUEUES * grid.items, 0), started((size_t)grid.blocks, 0) {}

    void maybe_run_others()
    {
        if (!rng || depth >= 3)
            return;
        while (!pending.empty() && (*rng)() % 3 == 0) {
            const size_t i = (*rng)() % pending.size();
            const int b = pending[i];
            pending[i] = pending.back();
            pending.pop_back();
            run(b);
        }
    }
    void run(int b)
    {
        if (started[(size_t)b])
            return;
        started[(size_t)b] = 1;
        depth++;
        int draws = 0;
        const int bid = lk_queue_take(
            b & 7, g.items,
            [&](int q) {
                maybe_run_others();
                draws++;
                return ctr[q]++;
            },
            [&](int q) {
                marks++;
                ctr[q] |= LKQ_ALL_DRY;
            });
        depth--;
        most_draws = std::max(most_draws, draws);
        if (bid < 0)
            none++;
        else if (bid >= LKQ_QUEUES * g.items)
            bad = true;
        else
            taken[(size_t)bid]++;
    }
};

static bool check(const char *what, int n_frames, int ppp, int div, Sim &s)
{
    const LkQueueGrid &g = s.g;
    bool ok = !s.bad && s.most_draws <= LKQ_QUEUES && s.none == LKQ_QUEUES * g.surplus && s.marks >= 1;
    for (char c : s.started)
        ok = ok && c;
    for (int t : s.taken)
        ok = ok && t == 1;
    // the items are the (frame slot, feature) pairs of the groups, each once
    const int groups = (n_frames + 7) / 8;
    std::vector<int> seen((size_t)groups * 8 * ppp, 0);
    for (int bid = 0; bid < LKQ_QUEUES * g.items; bid++) {
        const LkItem it = lk_block_item(bid, g.fpg, g.ppp);
        if (it.frame < 0 || it.frame >= groups * 8 || it.f < 0 || it.f >= ppp)
            ok = false;
        else
            seen[(size_t)it.frame * ppp + it.f]++;
    }
    for (int v : seen)
        ok = ok && v == 1;
    if (!ok)
        printf("%s: n_frames %d ppp %d surplus 1/%d: without item %d (surplus %d), most draws %d, marks %d, bad id %d\n", what, n_frames, ppp,
               div, s.none, LKQ_QUEUES * g.surplus, s.most_draws, s.marks, (int)s.bad);
    return ok;
}

int main()
{
    int geometries = 0, orders = 0;
    for (int n_frames : {16, 17, 20, 24, 33})
        for (int ppp : {1, 5, 64})
            for (int div : {16, 8, 4}) {
                const LkQueueGrid g = lk_queue_grid(n_frames, ppp, div);
                if (g.fpg != 8 || g.ppp != ppp || g.items != (n_frames + 7) / 8 * ppp || g.surplus < 1 || g.blocks != 8 * (g.items + g.surplus)) {
                    printf("lk_queue_grid(%d, %d, %d)\n", n_frames, ppp, div);
                    return 1;
                }
                geometries++;
                { // dispatch order
                    Sim s(g);
                    for (int b = 0; b < g.blocks; b++)
                        s.run(b);
                    if (!check("dispatch order", n_frames, ppp, div, s))
                        return 1;
                }
                { // reverse
                    Sim s(g);
                    for (int b = g.blocks - 1; b >= 0; b--)
                        s.run(b);
                    if (!check("reverse order", n_frames, ppp, div, s))
                        return 1;
                }
                for (int x = 0; x < LKQ_QUEUES; x += 3) { // one XCD entirely first
                    Sim s(g);
                    for (int b = 0; b < g.blocks; b++)
                        if ((b & 7) == x)
                            s.run(b);
                    for (int b = 0; b < g.blocks; b++)
                        s.run(b);
                    if (!check("one XCD first", n_frames, ppp, div, s))
                        return 1;
                }
                orders += 5;
                for (int seed = 0; seed < 200; seed++) { // random interleavings
                    std::mt19937 rng((unsigned)(seed * 7919 + n_frames * 131 + ppp * 17 + div));
                    Sim s(g);
                    s.rng = &rng;
                    std::vector<int> order((size_t)g.blocks);
                    for (int b = 0; b < g.blocks; b++)
                        order[(size_t)b] = b;
                    std::shuffle(order.begin(), order.end(), rng);
                    s.pending = order;
                    for (int b : order)
                        s.run(b);
                    if (!check("random interleaving", n_frames, ppp, div, s))
                        return 1;
                    orders++;
                }
            }
    printf("OK %d %d\n", geometries, orders);
    return 0;
}
