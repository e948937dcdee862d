// The contractions of the Born operator's reciprocal mode (lsfc_born_contract; DESIGN.md section 3, "Reciprocal mode").  With the
// fields U (nsrc x N) and the receiver fields V = M^-1 R^T (nrecv x N), J and J^H need no solve:
//     OP_N   out[s, r] = scale sum_i (in[i] u_s[i]) v_r[i]
//     OP_H   out[i]    = [out[i] +] conj(scale) sum_s conj(u_s[i]) q_s[i],   q_s[i] = sum_r conj(v_r[i]) in[s, r]
// Both run on the fp64 matrix cores, v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], and register j of
// the result is D[(l >> 4) + 4 j][l & 15].  A lane loads whole complex numbers (16 B) and feeds their real and imaginary parts to
// separate instructions, so that no loaded byte is unused and no operand moves between lanes:
//   k_contract_n   one wave owns 16 sources x 16 receivers.  A step takes 4 points (k = l >> 4): the lane loads u_s[i], v_r[i] and
//                  in[i], forms w = in[i] u_s[i] and issues four instructions, (re w)(re v), (re w)(im v), (im w)(re v), (im w)(im v),
//                  each into its own 16 x 16 real accumulator.  The four waves of a block own consecutive quarters of the block's
//                  points and are added in wave order; the blocks' partials (a function of N alone) are summed in block order by
//                  k_contract_n_finish, which then combines the four real sums, re = rr - ii, im = ri + ir, once, and scales.
//                  Every out[s, r] is its own chain of multiply-adds in point order: its bits depend on u_s, v_r, in and N only.
//   k_contract_h   the residuals are the stationary operand: rows are 16 sources, columns 16 points, k runs over 4 receivers.  The
//                  lane loads in[s, r] and v_r[i]; q's real part takes (re in)(re v) and then (im in)(im v), its imaginary part
//                  (im in)(re v) and then (-re in)(im v), receiver quads in order.  A lane then holds q of sources g, g + 4, g + 8,
//                  g + 12 (g = l >> 4) at its point, multiplies by conj(u_s) and sums them in that order; the four lanes of a point
//                  add (g0 + g1) + (g2 + g3); conj(scale) times that goes onto the running value of out[i].  One launch per 16
//                  sources, in order: a cut at a multiple of 16 sources through LSFC_BORN_ACCUMULATE gives the bits of one call.
// Members and points beyond the counts are zero operands made in registers; nothing is padded in memory.  No atomics, no LDS in
// the streaming loops (12 KB for the wave sum of k_contract_n), no scratch.
#include "plan.hpp"
#include "born_contract.hpp"
#include "reduce.hpp"
#include <algorithm>

namespace lsfc {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int CT = CONTRACT_TILE;
constexpr int CN_THREADS = 256, CN_WAVES = CN_THREADS / 64;
constexpr int CN_STEP = 8;                        // points of one loop trip of a wave: two instructions' worth, loads issued together
constexpr int CN_PART = 4 * CT * CT;              // doubles of one block's partial: four real 16 x 16 sums
constexpr int CF_CHAINS = 4, CF_THREADS = 64 * 4 * CF_CHAINS;
constexpr int CH_THREADS = 256, CH_COLS = 32;     // points of one loop trip of a wave: two column groups share the residual loads

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ cplx load_or_zero(const cplx* p, bool ok) { return ok ? *p : make_double2(0.0, 0.0); }

// points of a block of k_contract_n and the number of such blocks: functions of N alone
inline int contract_blocks(int64_t N) {
    const int64_t b = (N + CONTRACT_BLOCK_POINTS - 1) / CONTRACT_BLOCK_POINTS;
    return (int)std::max<int64_t>(1, std::min<int64_t>(b, CONTRACT_BLOCKS));
}
inline int64_t contract_block_points(int64_t N) {
    const int64_t nb = contract_blocks(N), unit = CN_WAVES * CN_STEP;
    return ((N + nb - 1) / nb + unit - 1) / unit * unit;
}

// part[(tile nb + block) CN_PART + (q 4 + j) 64 + lane], q = rr, ri, ir, ii: the block's sums over its points.
// One launch index per (block of points, tile), the tiles of a block of points next to each other, and -- when the count allows --
// dealt out so that the eight dies, which take launch indices round robin, each get a contiguous run of them: the tiles that re-read
// the same points of U or V then do so from the same L2, close in time.  The place of a partial does not depend on this.
template <bool CPLX> __global__ __launch_bounds__(CN_THREADS)
void k_contract_n(const cplx* __restrict__ u, const cplx* __restrict__ v, const double* __restrict__ in, double* __restrict__ part,
                  int64_t N, int nsrc, int nrecv, int ntr, int ntiles, int nb, int64_t block_points) {
    __shared__ double sh[CN_WAVES - 1][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, k = lane >> 4;
    const unsigned total = gridDim.x, work = total % 8 == 0 ? (blockIdx.x % 8) * (total / 8) + blockIdx.x / 8 : blockIdx.x;
    const int tile = (int)(work % (unsigned)ntiles), block = (int)(work / (unsigned)ntiles);
    const int s = (tile / ntr) * CT + m, r = (tile % ntr) * CT + m;
    const bool has_s = s < nsrc, has_r = r < nrecv;
    const cplx* up = u + (size_t)(has_s ? s : 0) * N;
    const cplx* vp = v + (size_t)(has_r ? r : 0) * N;
    const int64_t wave_points = block_points / CN_WAVES, first = (int64_t)block * block_points + wave * wave_points + k;
    d4 acc[4] = {};
    for (int64_t t = 0; t < wave_points; t += CN_STEP) {
        const int64_t i0 = first + t, i1 = i0 + 4;
        const bool ok0 = i0 < N, ok1 = i1 < N;
        const cplx a0 = load_or_zero(up + i0, has_s && ok0), a1 = load_or_zero(up + i1, has_s && ok1);
        const cplx b0 = load_or_zero(vp + i0, has_r && ok0), b1 = load_or_zero(vp + i1, has_r && ok1);
        cplx w0, w1;
        if constexpr (CPLX) {
            const cplx* x = reinterpret_cast<const cplx*>(in);
            w0 = cprod(load_or_zero(x + i0, ok0), a0); w1 = cprod(load_or_zero(x + i1, ok1), a1);
        } else {
            const double x0 = ok0 ? in[i0] : 0.0, x1 = ok1 ? in[i1] : 0.0;
            w0 = make_double2(x0 * a0.x, x0 * a0.y); w1 = make_double2(x1 * a1.x, x1 * a1.y);
        }
        acc[0] = mfma(w0.x, b0.x, acc[0]); acc[1] = mfma(w0.x, b0.y, acc[1]); acc[2] = mfma(w0.y, b0.x, acc[2]); acc[3] = mfma(w0.y, b0.y, acc[3]);
        acc[0] = mfma(w1.x, b1.x, acc[0]); acc[1] = mfma(w1.x, b1.y, acc[1]); acc[2] = mfma(w1.y, b1.x, acc[2]); acc[3] = mfma(w1.y, b1.y, acc[3]);
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sh[wave - 1][e][lane] = acc[e >> 2][e & 3];
    }
    __syncthreads();
    if (wave == 0) {
        double* p = part + ((size_t)tile * nb + block) * CN_PART + lane;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            double t = acc[e >> 2][e & 3];
#pragma unroll
            for (int w = 0; w < CN_WAVES - 1; ++w) t += sh[w][e][lane];
            p[e * 64] = t;
        }
    }
}

// the second level: CF_CHAINS interleaved chains over the blocks, added in chain order; then the one combination of the four real sums
__global__ __launch_bounds__(CF_THREADS)
void k_contract_n_finish(const double* __restrict__ part, int nb, cplx scale, cplx* __restrict__ out, int nsrc, int nrecv, int ntr) {
    __shared__ double sh[CF_CHAINS][4][64];
    const int lane = threadIdx.x & 63, q = (threadIdx.x >> 6) & 3, c = threadIdx.x >> 8;
    const int tile = blockIdx.x, j = blockIdx.y;
    const double* p = part + (size_t)tile * nb * CN_PART + (q * 4 + j) * 64 + lane;
    double acc = 0.0;
#pragma unroll 8
    for (int b = c; b < nb; b += CF_CHAINS) acc += p[(size_t)b * CN_PART];
    sh[c][q][lane] = acc;
    __syncthreads();
    if (c == 0) {
#pragma unroll
        for (int w = 1; w < CF_CHAINS; ++w) acc += sh[w][q][lane];
        sh[0][q][lane] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int s = (tile / ntr) * CT + (lane >> 4) + 4 * j, r = (tile % ntr) * CT + (lane & 15);
        if (s < nsrc && r < nrecv)
            out[(size_t)s * nrecv + r] = cprod(scale, make_double2(sh[0][0][lane] - sh[0][3][lane], sh[0][1][lane] + sh[0][2][lane]));
    }
}

// sources s0 .. s0 + ns - 1 (ns <= 16) onto the running value of out; cs = conj(scale)
template <bool REAL> __global__ __launch_bounds__(CH_THREADS)
void k_contract_h(const cplx* __restrict__ u, const cplx* __restrict__ v, const cplx* __restrict__ in, double* out, cplx cs, int accumulate,
                  int64_t N, int s0, int ns, int nrecv) {
    const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
    const int64_t waves = (int64_t)gridDim.x * (CH_THREADS / 64), wave = (int64_t)blockIdx.x * (CH_THREADS / 64) + (threadIdx.x >> 6);
    const cplx* inp = in + (size_t)(s0 + (m < ns ? m : 0)) * nrecv;
    for (int64_t base = wave * CH_COLS; base < N; base += waves * CH_COLS) {
        const int64_t i0 = base + m, i1 = i0 + 16;
        const bool ok0 = i0 < N, ok1 = i1 < N;
        d4 qr0 = {}, qi0 = {}, qr1 = {}, qi1 = {};
        for (int r0 = 0; r0 < nrecv; r0 += 4) {
            const int r = r0 + g;
            const bool has_r = r < nrecv;
            const cplx a = load_or_zero(inp + r, has_r && m < ns);
            const cplx* vp = v + (size_t)(has_r ? r : 0) * N;
            const cplx b0 = load_or_zero(vp + i0, has_r && ok0), b1 = load_or_zero(vp + i1, has_r && ok1);
            qr0 = mfma(a.x, b0.x, qr0); qr0 = mfma(a.y, b0.y, qr0); qi0 = mfma(a.y, b0.x, qi0); qi0 = mfma(-a.x, b0.y, qi0);
            qr1 = mfma(a.x, b1.x, qr1); qr1 = mfma(a.y, b1.y, qr1); qi1 = mfma(a.y, b1.x, qi1); qi1 = mfma(-a.x, b1.y, qi1);
        }
        // conj(u_s) q_s of this lane's four sources, in source order
        cplx p0 = make_double2(0.0, 0.0), p1 = p0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = g + 4 * j;
            const cplx* up = u + (size_t)(s0 + (s < ns ? s : 0)) * N;
            const cplx c0 = load_or_zero(up + i0, s < ns && ok0), c1 = load_or_zero(up + i1, s < ns && ok1);
            cdot_acc(p0, c0, make_double2(qr0[j], qi0[j]));
            cdot_acc(p1, c1, make_double2(qr1[j], qi1[j]));
        }
        // (g0 + g1) + (g2 + g3) in every lane of a point
        p0.x += __shfl_xor(p0.x, 16, 64); p0.y += __shfl_xor(p0.y, 16, 64); p1.x += __shfl_xor(p1.x, 16, 64); p1.y += __shfl_xor(p1.y, 16, 64);
        p0.x += __shfl_xor(p0.x, 32, 64); p0.y += __shfl_xor(p0.y, 32, 64); p1.x += __shfl_xor(p1.x, 32, 64); p1.y += __shfl_xor(p1.y, 32, 64);
        // lanes of g = 0 write the first column group, lanes of g = 1 the second
        if (g < 2) {
            const int64_t i = g ? i1 : i0;
            const cplx p = g ? p1 : p0;
            if (i < N) {
                cplx acc = make_double2(0.0, 0.0);
                if (accumulate) { if constexpr (REAL) acc.x = out[i]; else acc = reinterpret_cast<const cplx*>(out)[i]; }
                acc = caddmul(acc, cs, p);
                if constexpr (REAL) out[i] = acc.x; else reinterpret_cast<cplx*>(out)[i] = acc;
            }
        }
    }
}

} // namespace

size_t contract_n_work(int64_t N, int64_t nsrc, int64_t nrecv) {
    return (size_t)((nsrc + CT - 1) / CT) * (size_t)((nrecv + CT - 1) / CT) * (size_t)contract_blocks(N) * CN_PART;
}

void contract_n_dev(hipStream_t st, const cplx* u, int64_t nsrc, const cplx* v, int64_t nrecv, const double* in, bool in_is_complex,
                    cplx* out, cplx scale, int64_t N, double* work) {
    const int nb = contract_blocks(N);
    const int64_t block_points = contract_block_points(N), nts = (nsrc + CT - 1) / CT, ntr = (nrecv + CT - 1) / CT;
    // at most 2^30 blocks in a launch: rows of source tiles, each tile's partials at its own place
    const int64_t rows = std::max<int64_t>(1, ((int64_t)1 << 30) / (ntr * nb));
    for (int64_t t0 = 0; t0 < nts; t0 += rows) {
        const int64_t cnt = std::min(rows, nts - t0), ns = std::min<int64_t>(cnt * CT, nsrc - t0 * CT);
        auto kern = in_is_complex ? k_contract_n<true> : k_contract_n<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(cnt * ntr * nb)), dim3(CN_THREADS), 0, st, u + t0 * CT * N, v, in, work, N, (int)ns, (int)nrecv, (int)ntr, (int)(cnt * ntr), nb, block_points);
        LSFC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_contract_n_finish, dim3((unsigned)(cnt * ntr), 4), dim3(CF_THREADS), 0, st, work, nb, scale, out + t0 * CT * nrecv, (int)ns, (int)nrecv, (int)ntr);
        LSFC_HIP(hipGetLastError());
    }
}

void contract_h_dev(hipStream_t st, const cplx* u, int64_t nsrc, const cplx* v, int64_t nrecv, const cplx* in, double* out, cplx scale,
                    bool accumulate, bool real, int64_t N) {
    const unsigned grid = grid_for(N, (CH_THREADS / 64) * CH_COLS, 2048);
    const cplx cs = make_double2(scale.x, -scale.y);
    for (int64_t s0 = 0; s0 < nsrc; s0 += CT) {
        const int ns = (int)std::min<int64_t>(CT, nsrc - s0);
        auto kern = real ? k_contract_h<true> : k_contract_h<false>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(CH_THREADS), 0, st, u + s0 * N, v, in + s0 * nrecv, out, cs, (accumulate || s0 > 0) ? 1 : 0, N, 0, ns, (int)nrecv);
        LSFC_HIP(hipGetLastError());
    }
}

} // namespace lsfc

using namespace lsfc;

extern "C" int lsfc_born_contract(lsfc_plan* plan, const double* u, int64_t nsrc, const double* v, int64_t nrecv, const double* in, int in_is_complex,
                                  double* out, int op, unsigned flags, double scale_re, double scale_im, int memspace) {
    return guarded([&] {
        LSFC_REQUIRE(plan && u && v && in && out, "lsfc_born_contract: NULL argument");
        LSFC_REQUIRE(nsrc >= 1 && nsrc < ((int64_t)1 << 31), "lsfc_born_contract: nsrc = %lld (at least 1)", (long long)nsrc);
        LSFC_REQUIRE(nrecv >= 1 && nrecv < ((int64_t)1 << 31), "lsfc_born_contract: nrecv = %lld (at least 1)", (long long)nrecv);
        LSFC_REQUIRE(op == LSFC_OP_N || op == LSFC_OP_T || op == LSFC_OP_H, "lsfc_born_contract: bad op %d (LSFC_OP_N or LSFC_OP_H)", op);
        LSFC_REQUIRE(op != LSFC_OP_T, "lsfc_born_contract: LSFC_OP_T is not offered (conj(H applied to conj(in)) for the caller who needs it)");
        LSFC_REQUIRE((flags & ~(LSFC_BORN_ACCUMULATE | LSFC_BORN_REAL)) == 0, "lsfc_born_contract: unknown flag in 0x%x (LSFC_BORN_ACCUMULATE | LSFC_BORN_REAL)", flags);
        LSFC_REQUIRE(flags == 0 || op == LSFC_OP_H, "lsfc_born_contract: LSFC_BORN_ACCUMULATE and LSFC_BORN_REAL go with LSFC_OP_H, not with LSFC_OP_N");
        LSFC_REQUIRE(in_is_complex == 0 || in_is_complex == 1, "lsfc_born_contract: in_is_complex = %d (0 or 1)", in_is_complex);
        LSFC_REQUIRE(op == LSFC_OP_N || in_is_complex == 1, "lsfc_born_contract: the input of LSFC_OP_H is nsrc x nrecv complex (in_is_complex = 1)");
        LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "lsfc_born_contract: bad memspace %d", memspace);
        LSFC_REQUIRE(!plan->multi, "lsfc_born_contract is not available on a multi-device plan");
        LSFC_REQUIRE(!plan->dist, "lsfc_born_contract is not available on a distributed (or simulated-rank) plan");
        LSFC_HIP(hipSetDevice(plan->device));
        const int64_t N = plan->N, nd = nsrc * nrecv;
        const bool host = memspace == LSFC_MEM_HOST, real = (flags & LSFC_BORN_REAL) != 0, acc = (flags & LSFC_BORN_ACCUMULATE) != 0;
        const cplx scale = make_double2(scale_re, scale_im);
        hipStream_t st = plan->stream;
        DevBuf<cplx> du, dv; DevBuf<double> din, dout;
        const size_t in_doubles = op == LSFC_OP_N ? (size_t)N * (in_is_complex ? 2 : 1) : (size_t)nd * 2;
        const size_t out_doubles = op == LSFC_OP_N ? (size_t)nd * 2 : (size_t)N * (real ? 1 : 2);
        const cplx *pu = (const cplx*)u, *pv = (const cplx*)v;
        const double* pin = in;
        double* pout = out;
        if (host) {
            du.alloc((size_t)(nsrc * N)); dv.alloc((size_t)(nrecv * N)); din.alloc(in_doubles); dout.alloc(out_doubles);
            LSFC_HIP(hipMemcpyAsync(du.p, u, du.bytes(), hipMemcpyHostToDevice, st));
            LSFC_HIP(hipMemcpyAsync(dv.p, v, dv.bytes(), hipMemcpyHostToDevice, st));
            LSFC_HIP(hipMemcpyAsync(din.p, in, din.bytes(), hipMemcpyHostToDevice, st));
            if (acc) LSFC_HIP(hipMemcpyAsync(dout.p, out, dout.bytes(), hipMemcpyHostToDevice, st));
            pu = du.p; pv = dv.p; pin = din.p; pout = dout.p;
        }
        if (op == LSFC_OP_N) {
            // the block partials live with the plan: successive calls are ordered on its stream (a larger request frees the old
            // buffer first, and hipFree waits for the device)
            const size_t need = contract_n_work(N, nsrc, nrecv);
            if (plan->contract_work.n < need) plan->contract_work.alloc(need);
            contract_n_dev(st, pu, nsrc, pv, nrecv, pin, in_is_complex != 0, (cplx*)pout, scale, N, plan->contract_work.p);
        } else {
            contract_h_dev(st, pu, nsrc, pv, nrecv, (const cplx*)pin, pout, scale, acc, real, N);
        }
        if (host) {
            LSFC_HIP(hipMemcpyAsync(out, dout.p, dout.bytes(), hipMemcpyDeviceToHost, st));
            LSFC_HIP(hipStreamSynchronize(st));
        }
    });
}
