// glint_steps.h -- the steps of the optimizer row pushes, one statement each (the contracts in
// include/glint_gpu.h): the step policies of the sliced fold (glint_rowstep.h) -- Adagrad, Adam,
// FTRL-proximal -- and the row scalars and update of row-wise Adagrad. Shared by the pushes of dense gradient
// rows (glint_rowadagrad.hip, glint_rowadam.hip, glint_rowftrl.hip, glint_rowadagrad_rowwise.hip) and their
// grouped forms (glint_rowstep_group.hip), so that the two cannot drift apart in a bit.
#pragma once
#include <cmath>

#include "glint_rowstep.h"

namespace glint {

// ---- Adagrad --------------------------------------------------------------------------------------
// The step policy of the sliced fold (glint_rowstep.h): one state part, h. lr and eps are rounded once to
// V on the host.
// The seven operations of the contract, each rounded on its own: hipcc would contract h + G * G into
// v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). u / d stays a division of the rounded lr * G
// -- G * (lr / d) rounds differently. sqrt and / are the compiler's IEEE ones (step_sqrt's note).
template <typename V>
struct AdagradScalars {
  static constexpr int kParts = 1;
  V lr, eps;
  __device__ __forceinline__ void step(V& w, V (&h)[1], V G) const {
#pragma clang fp contract(off)
    const V s = G * G;
    const V h2 = h[0] + s;
    const V r = step_sqrt(h2);
    const V d = r + eps;
    const V u = lr * G;
    const V p = u / d;
    const V w2 = w - p;
    h[0] = h2;
    w = w2;
  }
};

// ---- Adam -----------------------------------------------------------------------------------------
// The step policy of the sliced fold (glint_rowstep.h): two state parts, m and v, and the seven scalars of
// the contract, settled on the host in double and rounded once to V.
// The fourteen operations of the contract, each rounded on its own: hipcc would contract b1 * m + a1 * G
// and b2 * v + a2 * q into v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). r / rc2 and u / d
// stay divisions -- a multiplication by a reciprocal rounds differently. sqrt and / are the compiler's
// IEEE ones (step_sqrt's note).
template <typename V>
struct AdamScalars {
  static constexpr int kParts = 2;
  V b1, b2, a1, a2, alpha, rc2, eps;
  __device__ __forceinline__ void step(V& w, V (&mv)[2], V G) const {
#pragma clang fp contract(off)
    const V m = mv[0], v = mv[1];
    const V t1 = b1 * m;
    const V t2 = a1 * G;
    const V m2 = t1 + t2;
    const V q = G * G;
    const V t3 = b2 * v;
    const V t4 = a2 * q;
    const V v2 = t3 + t4;
    const V r = step_sqrt(v2);
    const V s = r / rc2;
    const V d = s + eps;
    const V u = alpha * m2;
    const V p = u / d;
    const V w2 = w - p;
    mv[0] = m2;
    mv[1] = v2;
    w = w2;
  }
};

// The scalars of one Adam call (step >= 1), settled here, once, in double, each rounded once to V.
template <typename V>
inline AdamScalars<V> adam_scalars(double lr, double beta1, double beta2, double eps, i64 step) {
  const double c1 = 1.0 - std::pow(beta1, (double)step), c2 = 1.0 - std::pow(beta2, (double)step);
  return {(V)beta1, (V)beta2, (V)(1.0 - beta1), (V)(1.0 - beta2), (V)(lr / c1), (V)std::sqrt(c2), (V)eps};
}

// ---- FTRL-proximal --------------------------------------------------------------------------------
__device__ __forceinline__ double ftrl_abs(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float ftrl_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double ftrl_copysign(double m, double s) { return __builtin_copysign(m, s); }
__device__ __forceinline__ float ftrl_copysign(float m, float s) { return __builtin_copysignf(m, s); }

// The step policy of the sliced fold (glint_rowstep.h): two state parts, z and n, and the four scalars of
// the contract, each rounded once to V on the host.
// The operations of the contract, each rounded on its own: hipcc would contract G - sg * w and n + G * G
// into v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). ds / alpha, b / alpha and y / d stay
// divisions -- a multiplication by a reciprocal rounds differently -- and r1 - r0 is the difference of two
// square roots, not q / (r1 + r0). sqrt and / are the compiler's IEEE ones (step_sqrt's note).
// The threshold is a select: both sides are computed and `a <= l1`, false for a NaN z', picks +0 or -e, so a
// NaN reaches w' through y. The quotient of the side not taken (d may be 0 there) is dropped unseen.
template <typename V>
struct FtrlScalars {
  static constexpr int kParts = 2;
  V alpha, beta, l1, l2;
  __device__ __forceinline__ void step(V& w, V (&zn)[2], V G) const {
#pragma clang fp contract(off)
    const V z = zn[0], n = zn[1];
    const V q = G * G;
    const V n2 = n + q;
    const V r0 = step_sqrt(n);
    const V r1 = step_sqrt(n2);
    const V ds = r1 - r0;
    const V sg = ds / alpha;
    const V t = sg * w;
    const V u = G - t;
    const V z2 = z + u;
    const V a = ftrl_abs(z2);
    const V s = ftrl_copysign(l1, z2);
    const V y = z2 - s;
    const V b = beta + r1;
    const V c = b / alpha;
    const V d = c + l2;
    const V e = y / d;
    const V w2 = a <= l1 ? V(0) : -e;
    zn[0] = z2;
    zn[1] = n2;
    w = w2;
  }
};

// ---- row-wise Adagrad -----------------------------------------------------------------------------
#ifndef GLINT_ROWWISE_KEEP_BUILD  // (a variant build for measurement sets 0: every row sums its run twice)
#define GLINT_ROWWISE_KEEP_BUILD GLINT_ROWWISE_KEEP_STRIPS
#endif
constexpr int kRowwiseKeep = GLINT_ROWWISE_KEEP_BUILD;  // strips kept in registers between the two passes

// The five row scalars of the contract, each rounded on its own; returns k and leaves h' in h. ss / C is
// a division, not a product with a reciprocal, and k = lr / d is one division per row. sqrt and / are the
// compiler's IEEE ones (step_sqrt's note, glint_rowstep.h).
template <typename V>
__device__ __forceinline__ V rowwise_scalars(V& h, V ss, V C, V lr, V eps) {
#pragma clang fp contract(off)
  const V s = ss / C;
  const V h2 = h + s;
  const V r = step_sqrt(h2);
  const V d = r + eps;
  const V k = lr / d;
  h = h2;
  return k;
}

// w' = w - (k * G), the product rounded before the subtraction: fma(-k, G, w) is not the contract's.
template <typename V>
__device__ __forceinline__ V rowwise_update(V w, V k, V G) {
#pragma clang fp contract(off)
  const V p = k * G;
  return w - p;
}

}  // namespace glint
