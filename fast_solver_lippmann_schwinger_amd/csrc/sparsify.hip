// Assembly of the sparsifying preconditioner's matrices on the device: buildSparseA*Conv / buildSparseAG*Conv
// (src/SparsifyingMatrix2D.jl, src/SparsifyingMatrix3D.jl) and Msp = As + omega^2 AG diag(nu)
// (examples/example.jl:67, examples/example3D.jl:61).  See DESIGN.md "Sparsifying matrices".
//
// Every grid point belongs to one stencil class (interior, faces, edges, corners).  For class c with sample sources
// S_c the reference takes a_c = U[:, end]' of svd(G[S_c, complement of S_c]) and stamps a_c (As) and a_c G[S_c, S_c]
// (AG) on the rows of its class.  Here:
//   1. k_gram: H_c = G_S G_S^H for all classes in one launch, rows gathered from the plan's spatial kernel (never
//      materialised), the columns of S_c masked, per-workgroup partials, a fixed-order second pass (k_sum_parts);
//   2. host: cyclic complex Jacobi of each H_c (at most 27 x 27);
//   3. k_refine: w_c = H_c u_c and |G_S^H u_c|^2 gathered again from the rows, one first-order correction of u_c
//      against the Jacobi basis (the Gram route squares the condition number; this step removes the squared part
//      of the error); the same pass returns |G_S^H u|^2 for the eigenvectors of the second smallest and the
//      largest eigenvalue: the three singular values reported are these Rayleigh quotients, summed with compensation;
//   4. k_gss: G[S_c, S_c] in the reference's entriesSparseG* source order, host: a_c G[S_c, S_c];
//   5. k_stamp: one thread per row writes the CSR row (closed-form rowptr, sorted columns) of As, AG and Msp.
#include "plan.hpp"
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

namespace lsfc {
namespace {

constexpr int MAXS = 27;                        // stencil entries of a class (3D interior)
constexpr int MAXP = MAXS * (MAXS + 1) / 2;     // upper-triangle entries of one Gram matrix
constexpr int GCOLS = 64;                       // columns per LDS tile
constexpr int GWG = 256;                        // threads per workgroup of the Gram kernels
constexpr int GPARTS = 256;                     // workgroups per class (partials of the first reduction)
constexpr int NVEC = 3;                         // vectors per class in the refinement pass: u of the smallest, the second smallest
                                                // and the largest eigenvalue of H_c
constexpr int RSLOT = MAXS + NVEC;              // refine partials per class: w[0..ns), then |G_S^H u_v|^2 for v < NVEC
static_assert(RSLOT <= 32, "k_refine: one lane of a group of 32 per slot");

enum { LO = 0, IN = 1, HI = 2 };

// per-axis position type of the 27 classes of src/SparsifyingMatrix3D.jl in the reference's order: interior, faces
// (x lo/hi, y lo/hi, z lo/hi), the twelve "vertex" edges, the eight corners (x fastest).  The 2D classes of
// src/SparsifyingMatrix2D.jl are entries 0-4 and 7-10 (interior, four edges, four corners) with z dropped.
const int kTypes[27][3] = {
    {IN, IN, IN},
    {LO, IN, IN}, {HI, IN, IN}, {IN, LO, IN}, {IN, HI, IN}, {IN, IN, LO}, {IN, IN, HI},
    {LO, LO, IN}, {HI, LO, IN}, {LO, HI, IN}, {HI, HI, IN},
    {LO, IN, LO}, {HI, IN, LO}, {LO, IN, HI}, {HI, IN, HI},
    {IN, LO, LO}, {IN, HI, LO}, {IN, LO, HI}, {IN, HI, HI},
    {LO, LO, LO}, {HI, LO, LO}, {LO, HI, LO}, {HI, HI, LO}, {LO, LO, HI}, {HI, LO, HI}, {LO, HI, HI}, {HI, HI, HI}};
const int k2dClasses[9] = {0, 1, 2, 3, 4, 7, 8, 9, 10};

// 2D stencils that do not follow the generic order (y fastest, offsets ascending per axis), as (dy, dx):
// the corners (1,m), (n,m) of entriesSparseA (:65-66, :88-100) and every entriesSparseG stencil (:221-262)
const int k2dA7[4][2] = {{0, 0}, {0, 1}, {-1, 0}, {-1, 1}};
const int k2dA8[4][2] = {{0, 0}, {0, -1}, {-1, 0}, {-1, -1}};
const int k2dG[9][9][2] = {
    {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}, {0, 0}, {1, 0}, {-1, 1}, {0, 1}, {1, 1}},
    {{0, 0}, {0, 1}, {1, 0}, {1, 1}, {-1, 0}, {-1, 1}},
    {{0, -1}, {0, 0}, {1, 0}, {1, -1}, {-1, 0}, {-1, -1}},
    {{0, -1}, {0, 0}, {0, 1}, {1, 0}, {1, 1}, {1, -1}},
    {{0, -1}, {0, 0}, {0, 1}, {-1, 0}, {-1, 1}, {-1, -1}},
    {{0, 0}, {0, 1}, {1, 0}, {1, 1}},
    {{0, 0}, {0, -1}, {1, 0}, {1, -1}},
    {{0, 0}, {0, 1}, {-1, 0}, {-1, 1}},
    {{0, 0}, {0, -1}, {-1, 0}, {-1, -1}}};

struct ClassDef {
    int type[3] = {IN, IN, IN};
    int ns = 0;
    int64_t base = 0;            // 0-based linear index of the sample point
    int64_t ofsA[MAXS];          // stencil offsets, entriesSparseA* order (also the placement offsets, Indices[c])
    int64_t ofsG[MAXS];          // the same stencil in entriesSparseG* order
};

struct Geometry {
    int64_t n = 0, m = 0, l = 0, N = 0;
    int ndim = 0, nclass = 0;
    std::vector<ClassDef> cls;
    int cls_of[27];              // tx + 3 ty + 9 tz -> class
};

inline int64_t half_even(int64_t n) {    // Julia round(Integer, n/2): ties to even
    if (n % 2 == 0) return n / 2;
    const int64_t k = (n - 1) / 2;
    return (k % 2 == 0) ? k : k + 1;
}

void axis_offsets(int t, int* o, int* cnt) {
    if (t == LO) { o[0] = 0; o[1] = 1; *cnt = 2; }
    else if (t == HI) { o[0] = -1; o[1] = 0; *cnt = 2; }
    else { o[0] = -1; o[1] = 0; o[2] = 1; *cnt = 3; }
}

// the class tables of the reference, restated (LSFC_EINVAL for unsupported grids)
Geometry make_geometry(int64_t n, int64_t m, int64_t l) {
    LSFC_REQUIRE(n >= 3 && m >= 3 && (l == 1 || l >= 3), "sparsify: every axis needs at least 3 points (got %lld x %lld x %lld)",
                 (long long)n, (long long)m, (long long)l);
    Geometry g;
    g.n = n; g.m = m; g.l = l; g.N = n * m * l;
    g.ndim = (l == 1) ? 2 : 3;
    for (int& v : g.cls_of) v = -1;
    if (g.ndim == 2) {
        LSFC_REQUIRE(n % 2 == 1 && m % 2 == 1, "sparsify: 2D needs odd n and m (src/SparsifyingMatrix2D.jl:7), got %lld x %lld",
                     (long long)n, (long long)m);
        g.nclass = 9;
        const int64_t N = g.N;
        // sample points, literally as src/SparsifyingMatrix2D.jl:20-66 (1-based there)
        const int64_t base[9] = {n * (m - 1) / 2 + (n + 1) / 2 - 1, n * (m - 1) / 2, n * (m - 1) / 2 - 1, (n + 1) / 2 - 1,
                                 N - (n + 1) / 2 - 1, 0, n - 1, n * m - n, n * m - 1};
        for (int c = 0; c < 9; ++c) {
            ClassDef d;
            const int* t = kTypes[k2dClasses[c]];
            d.type[0] = t[0]; d.type[1] = t[1]; d.type[2] = IN;
            d.base = base[c];
            if (c == 7 || c == 8) {
                const int (*s)[2] = (c == 7) ? k2dA7 : k2dA8;
                d.ns = 4;
                for (int i = 0; i < 4; ++i) d.ofsA[i] = s[i][0] * n + s[i][1];
            } else {
                int ox[3], oy[3], cx, cy;
                axis_offsets(t[0], ox, &cx); axis_offsets(t[1], oy, &cy);
                for (int a = 0; a < cx; ++a)          // IndRelative[r, c][:]: y (row) fastest
                    for (int b = 0; b < cy; ++b) d.ofsA[d.ns++] = oy[b] * n + ox[a];
            }
            for (int i = 0; i < d.ns; ++i) d.ofsG[i] = k2dG[c][i][0] * n + k2dG[c][i][1];
            g.cls_of[t[0] + 3 * t[1] + 9 * IN] = c;
            g.cls.push_back(d);
        }
    } else {
        g.nclass = 27;
        const int64_t half[3] = {half_even(n), half_even(m), half_even(l)};
        const int64_t len[3] = {n, m, l};
        for (int c = 0; c < 27; ++c) {
            ClassDef d;
            int64_t pos[3];
            int o[3][3], cnt[3];
            for (int a = 0; a < 3; ++a) {
                d.type[a] = kTypes[c][a];
                pos[a] = d.type[a] == LO ? 0 : d.type[a] == HI ? len[a] - 1 : half[a] - 1;
                axis_offsets(d.type[a], o[a], &cnt[a]);
            }
            d.base = pos[0] + n * (pos[1] + m * pos[2]);   // changeInd3D (src/SparsifyingMatrix3D.jl:7-11)
            for (int z = 0; z < cnt[2]; ++z)               // Ind_relative[ii, jj, kk][:]: x fastest
                for (int y = 0; y < cnt[1]; ++y)
                    for (int x = 0; x < cnt[0]; ++x) d.ofsA[d.ns++] = o[0][x] + n * (o[1][y] + m * o[2][z]);
            for (int i = 0; i < d.ns; ++i) d.ofsG[i] = d.ofsA[i];   // entriesSparseG3D: same sources, same order
            g.cls_of[d.type[0] + 3 * d.type[1] + 9 * d.type[2]] = c;
            g.cls.push_back(d);
        }
    }
    return g;
}

// closed-form CSR row start of grid point (i0, i1, i2): rows are stored in grid order, a point has
// w(type x) w(type y) w(type z) entries (w = 3 inside, 2 on a boundary; the 2D z axis counts 1)
__host__ __device__ inline int64_t prefix_w(int64_t i) { return i == 0 ? 0 : 2 + 3 * (i - 1); }
__host__ __device__ inline int axis_type(int64_t i, int64_t n) { return i == 0 ? LO : (i == n - 1 ? HI : IN); }
__host__ __device__ inline int64_t row_start3(int64_t i0, int64_t i1, int64_t i2, int64_t n, int64_t m, int64_t l, int ndim) {
    const int64_t Wx = 3 * n - 2, Wy = 3 * m - 2;
    const int64_t wy = axis_type(i1, m) == IN ? 3 : 2;
    const int64_t wz = ndim == 2 ? 1 : (axis_type(i2, l) == IN ? 3 : 2);
    const int64_t pz = ndim == 2 ? 0 : prefix_w(i2);
    return pz * Wx * Wy + prefix_w(i1) * Wx * wz + prefix_w(i0) * wy * wz;
}
inline int64_t total_nnz(const Geometry& g) {
    return (3 * g.n - 2) * (3 * g.m - 2) * (g.ndim == 2 ? 1 : 3 * g.l - 2);
}

// ---- device side ---------------------------------------------------------------------------------------------------
struct DevClass {
    int ns, np;
    int64_t src[MAXS];           // linear indices of the sample sources (A order)
    int sx[MAXS], sy[MAXS], sz[MAXS];
    int gx[MAXS], gy[MAXS], gz[MAXS];      // sources in entriesSparseG* order
    unsigned short pr[MAXP];     // (a << 8) | b, a <= b
};

struct StampClass {
    int ns;
    int64_t ofs[MAXS];           // placement offsets, ascending
    cplx a[MAXS], ag[MAXS];      // As and AG values in that order
};

__device__ inline cplx kat(const cplx* __restrict__ K, int64_t j, int sx, int sy, int sz, int n, int m) {
    const int64_t nm = (int64_t)n * m;
    const int i0 = (int)(j % n), i1 = (int)((j / n) % m), i2 = (int)(j / nm);
    return K[abs(i0 - sx) + (int64_t)n * (abs(i1 - sy) + (int64_t)m * abs(i2 - sz))];
}

// one LDS tile: T[col][s] = G[src_s, j0 + col], zero where j0 + col is past N or one of the class's sources
__device__ inline void gather_tile(const cplx* __restrict__ K, const DevClass& C, int ns, int64_t j0, int64_t N, int n, int m,
                                   cplx (*T)[MAXS], int* masked) {
    const int tid = threadIdx.x;
    if (tid < GCOLS) {
        const int64_t j = j0 + tid;
        int mk = j >= N;
        for (int t = 0; t < ns; ++t) mk |= (C.src[t] == j);
        masked[tid] = mk;
    }
    __syncthreads();
    for (int e = tid; e < ns * GCOLS; e += GWG) {
        const int col = e % GCOLS, s = e / GCOLS;
        cplx v = make_double2(0.0, 0.0);
        if (!masked[col]) v = kat(K, j0 + col, C.sx[s], C.sy[s], C.sz[s], n, m);
        T[col][s] = v;
    }
    __syncthreads();
}

__device__ inline void cmac_conj(cplx& acc, cplx x, cplx y) {     // acc += x * conj(y)
    acc.x = fma(x.x, y.x, fma(x.y, y.y, acc.x));
    acc.y = fma(x.y, y.x, fma(-x.x, y.y, acc.y));
}

// H_c (upper triangle) partials: part[(c * gridDim.x + g) * MAXP + p]
__global__ __launch_bounds__(GWG) void k_gram(const cplx* __restrict__ K, const DevClass* __restrict__ cls, cplx* __restrict__ part,
                                             int n, int m, int64_t N, int64_t nchunks) {
    __shared__ cplx T[GCOLS][MAXS];
    __shared__ int masked[GCOLS];
    const int c = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const DevClass& C = cls[c];
    const int ns = C.ns, np = C.np;
    const bool h0 = tid < np, h1 = tid + GWG < np;
    const int p0 = h0 ? C.pr[tid] : 0, p1 = h1 ? C.pr[tid + GWG] : 0;
    const int a0 = p0 >> 8, b0 = p0 & 255, a1 = p1 >> 8, b1 = p1 & 255;
    cplx acc0 = make_double2(0.0, 0.0), acc1 = make_double2(0.0, 0.0);
    for (int64_t q = g; q < nchunks; q += gridDim.x) {
        gather_tile(K, C, ns, q * GCOLS, N, n, m, T, masked);
        if (h0) for (int col = 0; col < GCOLS; ++col) cmac_conj(acc0, T[col][a0], T[col][b0]);
        if (h1) for (int col = 0; col < GCOLS; ++col) cmac_conj(acc1, T[col][a1], T[col][b1]);
        __syncthreads();
    }
    cplx* out = part + ((int64_t)c * gridDim.x + g) * MAXP;
    if (h0) out[tid] = acc0;
    if (h1) out[tid + GWG] = acc1;
}

// compensated summation: a sum of n positive terms keeps a relative error of about 2 eps whatever n is
__device__ inline void kahan_add(double& sum, double& comp, double x) {
    const double y = x - comp, t = sum + y;
    comp = (t - sum) - y;
    sum = t;
}

// refinement partials, for the NVEC vectors u_v of a class (u[(v * nclass + c) * MAXS + s]): y_vj = sum_s conj(u_vs) G[src_s, j];
// for v = 0 (the smallest eigenvalue) w_s = sum_j G[src_s, j] conj(y_0j) (= (H u_0)_s); for every v the Rayleigh quotient
// sum_j |y_vj|^2 = |G_S^H u_v|^2, which is the squared singular value to second order in the error of u_v: the eigenvalues of
// the Gram matrix themselves are off by eps sigma_max^2, which is eps sigma_max (sigma_max / sigma) in sigma.
// part[(c * gridDim.x + g) * RSLOT + s], slot ns + v = |y_v|^2.  Thread (s = tid % 32, column group tid / 32).
__global__ __launch_bounds__(GWG) void k_refine(const cplx* __restrict__ K, const DevClass* __restrict__ cls, const cplx* __restrict__ u,
                                               cplx* __restrict__ part, int n, int m, int64_t N, int64_t nchunks) {
    __shared__ cplx T[GCOLS][MAXS];
    __shared__ cplx Y[NVEC][GCOLS];
    __shared__ cplx red[GWG / 32][RSLOT];
    __shared__ int masked[GCOLS];
    const int c = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const DevClass& C = cls[c];
    const int ns = C.ns, s = tid % 32, cg = tid / 32;
    const int nclass = gridDim.y;
    cplx accw = make_double2(0.0, 0.0);
    double accy = 0.0, compy = 0.0;
    for (int64_t q = g; q < nchunks; q += gridDim.x) {
        gather_tile(K, C, ns, q * GCOLS, N, n, m, T, masked);
        if (tid < NVEC * GCOLS) {
            const int v = tid / GCOLS, col = tid % GCOLS;
            const cplx* uv = u + ((int64_t)v * nclass + c) * MAXS;
            cplx y = make_double2(0.0, 0.0);
            for (int t = 0; t < ns; ++t) cmac_conj(y, T[col][t], uv[t]);      // conj(u_t) T[col][t]
            Y[v][col] = y;
        }
        __syncthreads();
        for (int col = cg; col < GCOLS; col += GWG / 32) {
            if (s < ns) cmac_conj(accw, T[col][s], Y[0][col]);
            else if (s < ns + NVEC) { const cplx y = Y[s - ns][col]; kahan_add(accy, compy, fma(y.x, y.x, y.y * y.y)); }
        }
        __syncthreads();
    }
    if (s < ns) red[cg][s] = accw;
    else if (s < ns + NVEC) red[cg][s] = make_double2(accy, 0.0);
    __syncthreads();
    if (tid < ns + NVEC) {
        cplx v = make_double2(0.0, 0.0), e = make_double2(0.0, 0.0);
        for (int k = 0; k < GWG / 32; ++k) { kahan_add(v.x, e.x, red[k][tid].x); kahan_add(v.y, e.y, red[k][tid].y); }    // fixed order
        part[((int64_t)c * gridDim.x + g) * RSLOT + tid] = v;
    }
}

// out[c * slots + p] = sum over g (in order, compensated) of part[(c * G + g) * slots + p]
__global__ void k_sum_parts(const cplx* __restrict__ part, cplx* __restrict__ out, int G, int slots, int nclass) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nclass * slots) return;
    const int c = idx / slots, p = idx % slots;
    cplx v = make_double2(0.0, 0.0), e = make_double2(0.0, 0.0);
    for (int g = 0; g < G; ++g) { const cplx w = part[((int64_t)c * G + g) * slots + p]; kahan_add(v.x, e.x, w.x); kahan_add(v.y, e.y, w.y); }
    out[idx] = v;
}

// G[S_c, S_c] in entriesSparseG* order: out[(c * MAXS + i) * MAXS + j]
__global__ void k_gss(const cplx* __restrict__ K, const DevClass* __restrict__ cls, cplx* __restrict__ out, int n, int m, int nclass) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nclass * MAXS * MAXS) return;
    const int c = idx / (MAXS * MAXS), i = (idx / MAXS) % MAXS, j = idx % MAXS;
    const DevClass& C = cls[c];
    if (i >= C.ns || j >= C.ns) return;
    out[idx] = K[abs(C.gx[i] - C.gx[j]) + (int64_t)n * (abs(C.gy[i] - C.gy[j]) + (int64_t)m * abs(C.gz[i] - C.gz[j]))];
}

__global__ void k_stamp(const StampClass* __restrict__ cls, const int* __restrict__ cls_of, int64_t n, int64_t m, int64_t l, int ndim,
                        int64_t nnz, const double* __restrict__ nu, const double* __restrict__ nu_im, double w2, int64_t* __restrict__ rowptr, int64_t* __restrict__ col,
                        cplx* __restrict__ As, cplx* __restrict__ AG, cplx* __restrict__ Msp) {
    const int64_t N = n * m * l;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = r % n, i1 = (r / n) % m, i2 = r / (n * m);
        const int tz = ndim == 2 ? IN : axis_type(i2, l);
        const StampClass& C = cls[cls_of[axis_type(i0, n) + 3 * axis_type(i1, m) + 9 * tz]];
        const int64_t rp = row_start3(i0, i1, i2, n, m, l, ndim);
        if (rowptr) { rowptr[r] = rp; if (r == N - 1) rowptr[N] = nnz; }
        for (int t = 0; t < C.ns; ++t) {
            const int64_t e = rp + t, j = r + C.ofs[t];
            if (col) col[e] = j;
            if (As) As[e] = C.a[t];
            if (AG) AG[e] = C.ag[t];
            if (Msp && nu_im) {          // complex nu (nu_im a kernel argument, null for real nu): a + (w2 nu[j]) * ag, a complex multiply-add
                const double fr = w2 * nu[j], fi = w2 * nu_im[j];
                Msp[e] = make_double2(fma(-fi, C.ag[t].y, fma(fr, C.ag[t].x, C.a[t].x)), fma(fi, C.ag[t].x, fma(fr, C.ag[t].y, C.a[t].y)));
            } else if (Msp) { const double f = w2 * nu[j]; Msp[e] = make_double2(C.a[t].x + f * C.ag[t].x, C.a[t].y + f * C.ag[t].y); }
        }
    }
}

// ---- host linear algebra --------------------------------------------------------------------------------------------
using zc = std::complex<double>;

// cyclic Jacobi of a Hermitian ns x ns matrix (row-major, overwritten): eigenvalues lam (unsorted), eigenvectors V (columns)
void jacobi_herm(int ns, std::vector<zc>& A, std::vector<double>& lam, std::vector<zc>& V) {
    V.assign((size_t)ns * ns, zc(0.0));
    for (int i = 0; i < ns; ++i) V[i * ns + i] = 1.0;
    auto at = [&](int i, int j) -> zc& { return A[(size_t)i * ns + j]; };
    double fro = 0.0;
    for (auto& v : A) fro += std::norm(v);
    fro = std::sqrt(fro);
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < ns; ++p) for (int q = p + 1; q < ns; ++q) off += std::norm(at(p, q));
        if (std::sqrt(off) <= 1e-18 * fro || off == 0.0) break;
        for (int p = 0; p < ns; ++p)
            for (int q = p + 1; q < ns; ++q) {
                const double r = std::abs(at(p, q));
                if (r == 0.0) continue;
                // phase: column q times e, row q times conj(e), so that A[p][q] becomes real positive
                const zc e = std::conj(at(p, q)) / r;
                for (int k = 0; k < ns; ++k) at(k, q) *= e;
                for (int k = 0; k < ns; ++k) at(q, k) *= std::conj(e);
                for (int k = 0; k < ns; ++k) V[(size_t)k * ns + q] *= e;
                at(p, q) = r; at(q, p) = r;
                const double app = at(p, p).real(), aqq = at(q, q).real();
                const double tau = (aqq - app) / (2.0 * r);
                const double t = (tau >= 0 ? 1.0 : -1.0) / (std::abs(tau) + std::sqrt(1.0 + tau * tau));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
                for (int k = 0; k < ns; ++k) {            // A J
                    const zc x = at(k, p), y = at(k, q);
                    at(k, p) = cs * x - sn * y; at(k, q) = sn * x + cs * y;
                }
                for (int k = 0; k < ns; ++k) {            // J^T A
                    const zc x = at(p, k), y = at(q, k);
                    at(p, k) = cs * x - sn * y; at(q, k) = sn * x + cs * y;
                }
                at(p, q) = 0.0; at(q, p) = 0.0;
                for (int k = 0; k < ns; ++k) {            // V J
                    const zc x = V[(size_t)k * ns + p], y = V[(size_t)k * ns + q];
                    V[(size_t)k * ns + p] = cs * x - sn * y; V[(size_t)k * ns + q] = sn * x + cs * y;
                }
            }
    }
    lam.resize(ns);
    for (int i = 0; i < ns; ++i) lam[i] = at(i, i).real();
}

void check_space(const void* ptr, int memspace, const char* name) {
    if (!ptr) return;
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, ptr);
    (void)hipGetLastError();
    const bool dev = e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
    const bool host_ok = !(e == hipSuccess && at.type == hipMemoryTypeDevice);
    if (memspace == LSFC_MEM_DEVICE) LSFC_REQUIRE(dev, "sparsify: %s is not device memory (memspace = LSFC_MEM_DEVICE)", name);
    else LSFC_REQUIRE(host_ok, "sparsify: %s is device memory (memspace = LSFC_MEM_HOST)", name);
}

void sparsify_build(lsfc_plan* p, int64_t* rowptr, int64_t* col, cplx* As, cplx* AG, cplx* Msp, double* sigma, int memspace) {
    LSFC_REQUIRE(p, "NULL plan");
    LSFC_REQUIRE(!p->dist && !p->multi, "sparsify: not available on a distributed or multi-device plan");
    LSFC_REQUIRE(memspace == LSFC_MEM_HOST || memspace == LSFC_MEM_DEVICE, "sparsify: memspace must be LSFC_MEM_HOST or LSFC_MEM_DEVICE");
    const Geometry g = make_geometry(p->dims[0], p->dims[1], p->ndim == 2 ? 1 : p->dims[2]);
    for (const ClassDef& d : g.cls) {
        LSFC_REQUIRE(g.N >= 2 * d.ns, "sparsify: grid of %lld points is too small for a stencil of %d sources", (long long)g.N, d.ns);
        for (int i = 0; i < d.ns; ++i) {
            LSFC_REQUIRE(d.base + d.ofsA[i] >= 0 && d.base + d.ofsA[i] < g.N, "sparsify: sample source outside the grid");
            for (int j = 0; j < i; ++j) LSFC_REQUIRE(d.ofsA[i] != d.ofsA[j], "sparsify: repeated sample source");
        }
    }
    check_space(rowptr, memspace, "rowptr"); check_space(col, memspace, "col"); check_space(As, memspace, "As_val");
    check_space(AG, memspace, "AG_val"); check_space(Msp, memspace, "Msp_val"); check_space(sigma, memspace, "sigma");
    LSFC_HIP(hipSetDevice(p->device));
    plan_kernel0(p);
    plan_require_even_kernel(p, "sparsify");        // kat() below reads K[|i - s|]
    const int nc = g.nclass, n = (int)g.n, m = (int)g.m;
    const int64_t N = g.N, nnz = total_nnz(g);

    std::vector<DevClass> hc(nc);
    for (int c = 0; c < nc; ++c) {
        const ClassDef& d = g.cls[c];
        DevClass& h = hc[c];
        memset(&h, 0, sizeof h);
        h.ns = d.ns; h.np = d.ns * (d.ns + 1) / 2;
        for (int i = 0; i < d.ns; ++i) {
            const int64_t s = d.base + d.ofsA[i], t = d.base + d.ofsG[i];
            h.src[i] = s;
            h.sx[i] = (int)(s % n); h.sy[i] = (int)((s / n) % m); h.sz[i] = (int)(s / ((int64_t)n * m));
            h.gx[i] = (int)(t % n); h.gy[i] = (int)((t / n) % m); h.gz[i] = (int)(t / ((int64_t)n * m));
        }
        int q = 0;
        for (int a = 0; a < d.ns; ++a) for (int b = a; b < d.ns; ++b) h.pr[q++] = (unsigned short)((a << 8) | b);
    }
    hipStream_t st = p->stream;
    DevBuf<DevClass> dcls; dcls.alloc(nc);
    LSFC_HIP(hipMemcpyAsync(dcls.p, hc.data(), nc * sizeof(DevClass), hipMemcpyHostToDevice, st));
    const int64_t nchunks = (N + GCOLS - 1) / GCOLS;
    const int G = (int)std::min<int64_t>(GPARTS, nchunks);
    DevBuf<cplx> part; part.alloc((size_t)nc * G * MAXP);
    DevBuf<cplx> sums; sums.alloc((size_t)nc * MAXP);
    DevBuf<cplx> gss; gss.alloc((size_t)nc * MAXS * MAXS);
    hipLaunchKernelGGL(k_gram, dim3(G, nc), dim3(GWG), 0, st, p->kernel0.p, dcls.p, part.p, n, m, N, nchunks);
    LSFC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sum_parts, dim3((nc * MAXP + 255) / 256), dim3(256), 0, st, part.p, sums.p, G, MAXP, nc);
    LSFC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gss, dim3((nc * MAXS * MAXS + 255) / 256), dim3(256), 0, st, p->kernel0.p, dcls.p, gss.p, n, m, nc);
    LSFC_HIP(hipGetLastError());
    std::vector<cplx> hH((size_t)nc * MAXP), hG((size_t)nc * MAXS * MAXS);
    LSFC_HIP(hipMemcpyAsync(hH.data(), sums.p, hH.size() * sizeof(cplx), hipMemcpyDeviceToHost, st));
    LSFC_HIP(hipMemcpyAsync(hG.data(), gss.p, hG.size() * sizeof(cplx), hipMemcpyDeviceToHost, st));
    LSFC_HIP(hipStreamSynchronize(st));

    // eigenpairs of every H_c
    std::vector<std::vector<zc>> V(nc);
    std::vector<std::vector<double>> lam(nc);
    std::vector<int> order_min(nc);
    std::vector<cplx> hu((size_t)NVEC * nc * MAXS, make_double2(0.0, 0.0));      // [NVEC][nc][MAXS]: smallest, second smallest, largest
    for (int c = 0; c < nc; ++c) {
        const int ns = hc[c].ns;
        std::vector<zc> A((size_t)ns * ns);
        int q = 0;
        for (int a = 0; a < ns; ++a)
            for (int b = a; b < ns; ++b, ++q) {
                const zc v(hH[(size_t)c * MAXP + q].x, hH[(size_t)c * MAXP + q].y);
                A[(size_t)a * ns + b] = v; A[(size_t)b * ns + a] = std::conj(v);
            }
        for (int a = 0; a < ns; ++a) A[(size_t)a * ns + a] = A[(size_t)a * ns + a].real();
        jacobi_herm(ns, A, lam[c], V[c]);
        // the columns of V are products of a few thousand rotations and drift from unit norm by as many roundings; the Rayleigh
        // quotients of k_refine carry that factor squared, so it is taken out here
        for (int b = 0; b < ns; ++b) {
            long double t = 0.0L;
            for (int s = 0; s < ns; ++s) { const zc e = V[c][(size_t)s * ns + b]; t += (long double)e.real() * e.real() + (long double)e.imag() * e.imag(); }
            const double r = (double)(1.0L / sqrtl(t));
            for (int s = 0; s < ns; ++s) V[c][(size_t)s * ns + b] *= r;
        }
        std::vector<int> by(ns);
        for (int i = 0; i < ns; ++i) by[i] = i;
        std::stable_sort(by.begin(), by.end(), [&](int x, int y) { return lam[c][x] < lam[c][y]; });
        const int imin = by[0], pick[NVEC] = {by[0], by[1], by[ns - 1]};
        order_min[c] = imin;
        for (int v = 0; v < NVEC; ++v)
            for (int s = 0; s < ns; ++s) {
                const zc e = V[c][(size_t)s * ns + pick[v]];
                hu[((size_t)v * nc + c) * MAXS + s] = make_double2(e.real(), e.imag());
            }
    }
    // refinement pass: w = H u and |G_S^H u|^2 from the rows themselves
    DevBuf<cplx> du; du.alloc(hu.size());
    LSFC_HIP(hipMemcpyAsync(du.p, hu.data(), hu.size() * sizeof(cplx), hipMemcpyHostToDevice, st));
    DevBuf<cplx> part2; part2.alloc((size_t)nc * G * RSLOT);
    DevBuf<cplx> sums2; sums2.alloc((size_t)nc * RSLOT);
    LSFC_HIP(hipMemsetAsync(part2.p, 0, part2.bytes(), st));
    hipLaunchKernelGGL(k_refine, dim3(G, nc), dim3(GWG), 0, st, p->kernel0.p, dcls.p, du.p, part2.p, n, m, N, nchunks);
    LSFC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sum_parts, dim3((nc * RSLOT + 255) / 256), dim3(256), 0, st, part2.p, sums2.p, G, RSLOT, nc);
    LSFC_HIP(hipGetLastError());
    std::vector<cplx> hw((size_t)nc * RSLOT);
    LSFC_HIP(hipMemcpyAsync(hw.data(), sums2.p, hw.size() * sizeof(cplx), hipMemcpyDeviceToHost, st));
    LSFC_HIP(hipStreamSynchronize(st));

    std::vector<StampClass> hs(nc);
    std::vector<double> hsig((size_t)nc * 3);
    for (int c = 0; c < nc; ++c) {
        const int ns = hc[c].ns, imin = order_min[c];
        const std::vector<zc>& Vc = V[c];
        const double lmin = hw[(size_t)c * RSLOT + ns].x;               // |G_S^H u|^2
        // z = V^H w: column imin of V^H H V; first-order correction of u against the other eigenvectors
        std::vector<zc> unew((size_t)ns);
        for (int s = 0; s < ns; ++s) unew[s] = Vc[(size_t)s * ns + imin];
        for (int b = 0; b < ns; ++b) {
            if (b == imin) continue;
            zc z(0.0);
            for (int s = 0; s < ns; ++s) z += std::conj(Vc[(size_t)s * ns + b]) * zc(hw[(size_t)c * RSLOT + s].x, hw[(size_t)c * RSLOT + s].y);
            const double den = lmin - lam[c][b];
            if (den == 0.0) continue;
            const zc coef = z / den;
            for (int s = 0; s < ns; ++s) unew[s] += coef * Vc[(size_t)s * ns + b];
        }
        double nrm = 0.0;
        for (auto& v : unew) nrm += std::norm(v);
        nrm = std::sqrt(nrm);
        // a_c = U[:, end]' (conjugate); phase: the first entry of largest modulus (reference stencil order) real positive
        std::vector<zc> a((size_t)ns);
        int imax = 0;
        for (int s = 0; s < ns; ++s) { a[s] = std::conj(unew[s]) / nrm; if (std::abs(a[s]) > std::abs(a[imax])) imax = s; }
        const zc ph = std::conj(a[imax]) / std::abs(a[imax]);
        for (auto& v : a) v *= ph;
        a[imax] = std::abs(a[imax]);
        // AG row: a_c G[S_c, S_c] with G in entriesSparseG* order (Values[c] * Entries[c])
        std::vector<zc> ag((size_t)ns, zc(0.0));
        for (int j = 0; j < ns; ++j)
            for (int i = 0; i < ns; ++i) {
                const cplx gv = hG[((size_t)c * MAXS + i) * MAXS + j];
                ag[j] += a[i] * zc(gv.x, gv.y);
            }
        // CSR order: offsets ascending
        const ClassDef& d = g.cls[c];
        std::vector<int> perm(ns);
        for (int i = 0; i < ns; ++i) perm[i] = i;
        std::sort(perm.begin(), perm.end(), [&](int x, int y) { return d.ofsA[x] < d.ofsA[y]; });
        StampClass& sc = hs[c];
        memset(&sc, 0, sizeof sc);
        sc.ns = ns;
        for (int t = 0; t < ns; ++t) {
            sc.ofs[t] = d.ofsA[perm[t]];
            sc.a[t] = make_double2(a[perm[t]].real(), a[perm[t]].imag());
            sc.ag[t] = make_double2(ag[perm[t]].real(), ag[perm[t]].imag());
        }
        // singular values: the Rayleigh quotients of the refinement pass (k_refine), not the eigenvalues of the Gram matrix
        hsig[c * 3 + 0] = std::sqrt(std::max(hw[(size_t)c * RSLOT + ns + 2].x, 0.0));
        hsig[c * 3 + 1] = std::sqrt(std::max(hw[(size_t)c * RSLOT + ns + 1].x, 0.0));
        hsig[c * 3 + 2] = std::sqrt(std::max(lmin, 0.0));
    }

    // stamp
    DevBuf<StampClass> dst; dst.alloc(nc);
    DevBuf<int> dof; dof.alloc(27);
    LSFC_HIP(hipMemcpyAsync(dst.p, hs.data(), nc * sizeof(StampClass), hipMemcpyHostToDevice, st));
    LSFC_HIP(hipMemcpyAsync(dof.p, g.cls_of, sizeof g.cls_of, hipMemcpyHostToDevice, st));
    const bool host = memspace == LSFC_MEM_HOST;
    DevBuf<int64_t> trp, tcol;
    DevBuf<cplx> tas, tag, tmsp;
    int64_t* drp = rowptr; int64_t* dcol = col; cplx* das = As; cplx* dag = AG; cplx* dmsp = Msp;
    if (host) {
        if (rowptr) { trp.alloc(N + 1); drp = trp.p; }
        if (col) { tcol.alloc(nnz); dcol = tcol.p; }
        if (As) { tas.alloc(nnz); das = tas.p; }
        if (AG) { tag.alloc(nnz); dag = tag.p; }
        if (Msp) { tmsp.alloc(nnz); dmsp = tmsp.p; }
    }
    if (drp || dcol || das || dag || dmsp) {
        const int64_t blocks = std::min<int64_t>((N + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_stamp, dim3((unsigned)blocks), dim3(256), 0, st, dst.p, dof.p, g.n, g.m, g.l, g.ndim, nnz, p->nu.p, p->nu_im.p,
                           p->omega * p->omega, drp, dcol, das, dag, dmsp);
        LSFC_HIP(hipGetLastError());
    }
    const hipMemcpyKind down = hipMemcpyDeviceToHost;
    if (host) {
        if (rowptr) LSFC_HIP(hipMemcpyAsync(rowptr, drp, (N + 1) * sizeof(int64_t), down, st));
        if (col) LSFC_HIP(hipMemcpyAsync(col, dcol, nnz * sizeof(int64_t), down, st));
        if (As) LSFC_HIP(hipMemcpyAsync(As, das, nnz * sizeof(cplx), down, st));
        if (AG) LSFC_HIP(hipMemcpyAsync(AG, dag, nnz * sizeof(cplx), down, st));
        if (Msp) LSFC_HIP(hipMemcpyAsync(Msp, dmsp, nnz * sizeof(cplx), down, st));
    }
    if (sigma && host) std::copy(hsig.begin(), hsig.end(), sigma);
    if (sigma && !host) LSFC_HIP(hipMemcpyAsync(sigma, hsig.data(), hsig.size() * sizeof(double), hipMemcpyHostToDevice, st));
    LSFC_HIP(hipStreamSynchronize(st));
}

} // namespace
} // namespace lsfc

using namespace lsfc;

int lsfc_sparsify_pattern(int64_t n, int64_t m, int64_t l, int64_t* nnz, int64_t* rowptr, int64_t* col, int64_t* row_class) {
    return guarded([&] {
        LSFC_REQUIRE(nnz, "NULL nnz");
        const Geometry g = make_geometry(n, m, l);
        *nnz = total_nnz(g);
        if (!rowptr && !col && !row_class) return;
        std::vector<std::vector<int64_t>> sorted(g.nclass);
        for (int c = 0; c < g.nclass; ++c) {
            sorted[c].assign(g.cls[c].ofsA, g.cls[c].ofsA + g.cls[c].ns);
            std::sort(sorted[c].begin(), sorted[c].end());
        }
        int64_t e = 0;
        for (int64_t r = 0; r < g.N; ++r) {
            const int64_t i0 = r % n, i1 = (r / n) % m, i2 = r / (n * m);
            const int tz = g.ndim == 2 ? IN : axis_type(i2, l);
            const int c = g.cls_of[axis_type(i0, n) + 3 * axis_type(i1, m) + 9 * tz];
            if (row_class) row_class[r] = c;
            if (rowptr) rowptr[r] = e;
            if (col) for (int64_t o : sorted[c]) col[e++] = r + o;
            else e += (int64_t)sorted[c].size();
        }
        if (rowptr) rowptr[g.N] = e;
    });
}

int lsfc_sparsify_build(lsfc_plan* plan, int64_t* rowptr, int64_t* col, double* As_val, double* AG_val, double* Msp_val, double* sigma,
                        int memspace) {
    return guarded([&] {
        sparsify_build(plan, rowptr, col, (cplx*)As_val, (cplx*)AG_val, (cplx*)Msp_val, sigma, memspace);
    });
}
