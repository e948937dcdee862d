// The two contractions of the Born operator's reciprocal mode (born_contract.hip; DESIGN.md section 3, "Reciprocal mode"): with the
// fields U (nsrc x N) and the receiver fields V (nrecv x N) on the device,
//     OP_N   out[s, r] = scale sum_i (in[i] u_s[i]) v_r[i]
//     OP_H   out[i]    = [out[i] +] conj(scale) sum_s conj(u_s[i]) sum_r conj(v_r[i]) in[s, r]
#pragma once
#include "common.hpp"

namespace lsfc {

static constexpr int CONTRACT_TILE = 16;          // sources x receivers of one MFMA tile (OP_N), sources of one launch (OP_H)
static constexpr int CONTRACT_BLOCKS = 1024;      // most blocks along the points (OP_N): the first level of its sum
static constexpr int CONTRACT_BLOCK_POINTS = 4096; // fewest points of such a block

// doubles of device work space that contract_n_dev needs: the block partials of every tile
size_t contract_n_work(int64_t N, int64_t nsrc, int64_t nrecv);
// device pointers, stream-ordered; `work` holds contract_n_work doubles
void contract_n_dev(hipStream_t st, const cplx* u, int64_t nsrc, const cplx* v, int64_t nrecv, const double* in, bool in_is_complex,
                    cplx* out, cplx scale, int64_t N, double* work);
void contract_h_dev(hipStream_t st, const cplx* u, int64_t nsrc, const cplx* v, int64_t nrecv, const cplx* in, double* out, cplx scale,
                    bool accumulate, bool real, int64_t N);

} // namespace lsfc
