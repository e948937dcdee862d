// Host-side interface of pointwise.hip.
#pragma once
#include "common.hpp"

namespace lsfc {

// complex nu as the plan stores it: n (re, im) pairs -> the two planes re[n], im[n] (lsfc_plan_set_nu_complex)
void pw_split_planes(const cplx* pairs, double* re, double* im, int64_t n, hipStream_t);
// rocFFT pipelines: W = pad((nu ? nu : 1) .* (conj ? conj(x) : x)) ...  (nu_im: Im nu, with nu its real part; the factor of
// conj(x) is then nu itself and that of conj(W) below conj(nu): the conjugation is outermost, plan.hpp)
void pw_embed(const cplx* x, const double* nu, cplx* W, const int dims[3], const int pads[3], hipStream_t, bool conj = false,
              const double* nu_im = nullptr);
void pw_mul_inplace(cplx* W, const cplx* S, int64_t total, hipStream_t);
void pw_crop_axpy(const cplx* W, const cplx* x, cplx* y, double alpha, double beta, const int dims[3], const int pads[3],
                  const int off[3], hipStream_t, const double* nu = nullptr, bool conj = false, const double* nu_im = nullptr);   // ... y = alpha*x + beta * nu .* (conj) crop(W)
// unit-modulus probe vector number `which` and its conjugate, a function of the index only (the symmetry check of a plan)
void pw_probe(cplx* v, cplx* vbar, int64_t n, int which, hipStream_t);
// symbol preparation
void pw_roll_scale(const cplx* src, cplx* dst, const int p[3], const int s[3], double scale, hipStream_t);
void pw_resample_kernel(const cplx* src, cplx* dst, const int p[3], const int q[3], const int origin[3], const int nmax[3], double scale, hipStream_t);
void pw_wrap_crop(const cplx* src, cplx* dst, const int p[3], const int q[3], double scale, hipStream_t);
// 3D: tiles [xb0, xb0+ntiles) of the x' axis only (the symbol slab of one rank); 2D: whole symbol
void pw_permute_symbol(const cplx* G2, cplx* out, const int* px, const int* pyrow, const int* pz, const int L[3], int rows, int hz, int xb0, int ntiles, double scale, hipStream_t,
                       int srcLy = 0 /* rows per z plane of the source when it holds ky, kz >= 0 only (0: L[1]) */);
// max |G(k) - G(L-k)| / max |G| along `axis` of a natural-order symbol (1.0 if it contains NaN)
double pw_mirror_deviation(const cplx* G, const int L[3], int axis, hipStream_t);
void pw_scale(cplx* a, double s, int64_t total, hipStream_t);

void pw_gather_sources(const cplx* K, cplx* out, const int64_t* src, int nsrc, const int dims[3], hipStream_t);
// max |R[i] - K[i mirrored along the axes of mask]| / max |K| on the grid `dims` (1.0 if either holds NaN or Inf): R is the
// response to a unit source at the corner that is last along the axes of `mask` (bit a = axis a), K the one at index 0
double pw_corner_deviation(const cplx* R, const cplx* K, const int dims[3], int mask, hipStream_t);

} // namespace lsfc
