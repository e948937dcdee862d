// Off-grid sources and receivers (receivers.hip): the dense nrecv x N sampling operator R of lsfc_receivers_*, never stored.
#pragma once
#include "common.hpp"

namespace lsfc {

static constexpr int RECV_RT = 4;        // receivers (or far-field directions) whose sums one thread of the forward kernels keeps in registers
static constexpr int RECV_CHUNK = 64;    // receivers staged through LDS at a time by the T / H kernel
static constexpr int RECV_PASS = 256;    // receivers of one forward launch (bounds the block partials: members * RECV_PASS * RED_BLOCKS complex)

// loads this translation unit's code object on the current device (pruned.hip: pruned_warmup)
void warmup_receivers();
// the device an object lives on (born.hip checks it against the plan's)
int receivers_device(const lsfc_receivers* rc);

} // namespace lsfc
