// vo_lkqueue.h -- the work items of the LK chain kernels and how lk_circular_queue_kernel (lk.hip) hands them out.
//
// A launch of lk_circular_kernel is a list of work items numbered like its workgroups: item b belongs to XCD b & 7 (the
// dispatcher's round robin) and is feature lk_block_item(b).f of frame lk_block_item(b).frame, so that XCD x tracks the frames
// x, x + 8, x + 16, ... one after another out of its own L2.  That split is static: an XCD whose frames are cheap idles until the
// slowest one is done (profiles/r10_lk_xcd_queue.md).  The queue kernel keeps the numbering and draws the number instead: queue x
// holds the items 8 t + x, t = 0 .. items - 1, in the order the static launch runs them, a workgroup on XCD x takes tickets from
// queue x, and once that is dry from queue x + 1, x + 2, ... (mod 8).  A dry queue stays dry -- tickets only grow -- so a
// workgroup draws at most 8 times, waits for nothing and depends on no other workgroup's progress.  Everything here is plain
// C++ for the device, the CPU emulator and a g++ program alike (tests/host_check/lk_queue_host.cpp replays arrival orders).
#pragma once

#include "vo_isa.h"

namespace vo {

constexpr int LKQ_QUEUES = 8;       // one per XCD
constexpr int LKQ_STRIDE = 32;      // words between two counters: each on its own 128-byte line
constexpr int LKQ_SETS = 2;         // launch k draws from set k & 1 and zeroes the other one for launch k + 1
constexpr int LKQ_WORDS = LKQ_SETS * LKQ_QUEUES * LKQ_STRIDE;
constexpr int LKQ_MIN_FRAMES = 16;  // the queue kernel's batches: groups of 8 frames, at least two of them
#ifndef VO_LKQ_SURPLUS_DIV // (-D: the surplus sweep of profiles/r10_lk_xcd_queue.md)
#define VO_LKQ_SURPLUS_DIV 16
#endif
constexpr int LKQ_SURPLUS_DIV = VO_LKQ_SURPLUS_DIV; // surplus workgroups per XCD = ceil(items / 16): the best of 1/32 .. 1/4 on the headline
// set in an XCD's own counter once one of its workgroups has found all eight queues dry: see lk_queue_take.  Above every ticket
// a launch can reach (launch_lk_circular keeps items below 2^26, and a workgroup draws from a counter at most once).
constexpr unsigned LKQ_ALL_DRY = 1u << 30;

// work item `bid` of the block numbering: XCD bid & 7, slot bid >> 3 = (group of fpg frames, place in a part of ppp features)
struct LkItem {
    int frame, f;
};
VO_HD LkItem lk_block_item(int bid, int fpg, int ppp)
{
    const int xcd = bid & 7, slot = bid >> 3;
    const int grp = slot / ppp, fi = slot - grp * ppp;
    return LkItem{grp * fpg + (xcd & (fpg - 1)), (xcd / fpg) * ppp + fi};
}

// The draw / steal rule of a workgroup on XCD x.  draw(q) takes the next ticket of queue q (a fetch-and-add of 1, the same value
// for the whole workgroup).  Returns the work item's number, 8 t + q of the first queue from x on that still had a ticket below
// `items`, or -1 when all eight are dry.  The workgroup that finds them all dry says so in its OWN counter -- mark(x), an atomic
// OR of LKQ_ALL_DRY -- and every later workgroup of that XCD stops at its first draw: the surplus workgroups of a finished
// launch then touch one counter each, their XCD's, where eight draws each on the same eight addresses cost more than the idle
// XCDs did (profiles/r10_lk_xcd_queue.md, section 3).  To a workgroup of another XCD a marked counter is a dry queue, which it is.
template <typename Draw, typename Mark>
VO_HD int lk_queue_take(int x, int items, Draw &&draw, Mark &&mark)
{
    unsigned t = draw(x);
    if (t < (unsigned)items)
        return LKQ_QUEUES * (int)t + x;
    if (t >= LKQ_ALL_DRY)
        return -1;
    for (int k = 1; k < LKQ_QUEUES; k++) {
        const int q = (x + k) & (LKQ_QUEUES - 1);
        t = draw(q);
        if (t < (unsigned)items)
            return LKQ_QUEUES * (int)t + q;
    }
    mark(x);
    return -1;
}

// The queue kernel's launch geometry beside lk_grid's (lk.hip): fpg = 8, so a part is a frame's whole list (ppp = n_items) and
// every queue holds items = groups * ppp tickets.  Each XCD gets items + surplus workgroups: on a fast XCD the surplus is what
// takes work over, on the slowest it finds every queue dry and ends.
struct LkQueueGrid {
    int fpg, ppp, items, surplus, blocks;
};
inline LkQueueGrid lk_queue_grid(int n_frames, int n_items, int surplus_div = LKQ_SURPLUS_DIV)
{
    const int groups = (n_frames + 7) / 8, items = groups * n_items;
    const int surplus = (items + surplus_div - 1) / surplus_div;
    return {8, n_items, items, surplus, LKQ_QUEUES * (items + surplus)};
}

} // namespace vo
