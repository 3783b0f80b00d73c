// kernel_constants.h — what the host code that launches no kernel of kernels.h still needs to know of them: the block size
// and the counter slots (context.h, and through it every unit of the C ABI). kernels.h includes it.
#pragma once

#define STHIP_BLOCK 256

// counter slots in FrameParams::counters: they accumulate over a render call (queue sizes live in FrameParams::qctl)
enum {
  CNT_RAYS_CLOSEST = 0,
  CNT_RAYS_SHADOW = 1,
  CNT_NODES = 2,  // +1: shadow rays
  CNT_TRIS = 4,   // +1: shadow rays
  CNT_INNER_SLOTS = 6,  // +1: shadow rays
  CNT_TRI_SLOTS = 8,    // +1: shadow rays
  CNT_ROUND_SLOTS = 10, // +1: shadow rays: 64 per round of a persistent wave
  CNT_BUSY_ROUNDS = 12, // +1: shadow rays: lanes holding a ray, summed over rounds
  CNT_NODES_PRIMARY = 14,  // the share of CNT_NODES / CNT_TRIS that k_trace_primary (first bounce as wave packets) counted
  CNT_TRIS_PRIMARY = 15,
  CNT_CROSSINGS = 16,  // media: closest-hit queries that only carried a path across a volume boundary (no new trace() call)
  CNT_RAYS_ANSWERED = 17,  // of CNT_RAYS_CLOSEST: last rays of paths that k_shade answered from the emitters' bounds (never queued)
  CNT_LANE_STATES = 20,  // 8 slots: TraverseCounters::st
  CNT_TOTAL = 28
};
