// pdehip_pieces.h — VEC cells of a row in one access, for the analysis kernels: the loader (pdehip_stats.hip, pdehip_hist.hip,
// pdehip_project.hip, pdehip_smooth.hip) and the store (pdehip_stats.hip), the values of such a piece - the cells of one component, or
// the norm over the components (pdehip_stats.hip, pdehip_hist.hip) - and, on the host, the one rule for VEC (piece_width) and the one
// choice of the kernel instance <type, VEC> (dispatch_piece), which all four units use.
#pragma once

#include <type_traits>

#include "pdehip_common.h"

namespace pdehip {

// VEC cells of a row in one access (VEC > 1: the address is a multiple of 16 bytes - rows start on 128-byte lines, the callers check the
// base pointers)
template <typename T, int VEC>
__device__ __forceinline__ void load_piece(const T *p, T (&v)[VEC])
{
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else {
        typedef T vec_t __attribute__((ext_vector_type(VEC)));
        const vec_t x = *(const vec_t *)p;
#pragma unroll
        for (int q = 0; q < VEC; q++) v[q] = x[q];
    }
}
template <typename T, int VEC>
__device__ __forceinline__ void store_piece(T *p, const T (&v)[VEC])
{
    if constexpr (VEC == 1) {
        p[0] = v[0];
    } else {
        typedef T vec_t __attribute__((ext_vector_type(VEC)));
        vec_t x;
#pragma unroll
        for (int q = 0; q < VEC; q++) x[q] = v[q];
        *(vec_t *)p = x;
    }
}

// the values of one piece at `in`: the cells themselves, or s = sqrt(x_0 * x_0 + x_1 * x_1 + ...) over `ncomp` components `pc` elements
// apart, in the field's type, one rounding per operation
template <typename T, int VEC, bool NORM>
__device__ __forceinline__ void piece_values(const T *in, long pc, int ncomp, T (&v)[VEC])
{
    load_piece<T, VEC>(in, v);
    if (NORM) {
#pragma unroll
        for (int q = 0; q < VEC; q++) v[q] = v[q] * v[q];
        for (int c = 1; c < ncomp; c++) {
            T x[VEC];
            load_piece<T, VEC>(in + c * pc, x);
#pragma unroll
            for (int q = 0; q < VEC; q++) v[q] = v[q] + x[q] * x[q];
        }
#pragma unroll
        for (int q = 0; q < VEC; q++) v[q] = sqrt(v[q]);
    }
}

// cells per access: 16 bytes where the rows and the arrays allow
inline int piece_width(const NGrid &n, const void *a, const void *b)
{
    if ((((uintptr_t)a | (uintptr_t)b) & 15) != 0) return 1;
    if (n.dtype == PDEHIP_F64) return n.n[2] % 2 == 0 ? 2 : 1;
    return n.n[2] % 4 == 0 ? 4 : 1;
}

// fn(T(), std::integral_constant<int, VEC>()) for the one of <double, 2>, <double, 1>, <float, 4>, <float, 1> that `dtype` and the width
// of piece_width name: the caller's generic lambda launches its kernel instance <T, VEC>
template <class F>
inline void dispatch_piece(int dtype, int vec, F &&fn)
{
    if (dtype == PDEHIP_F64) {
        if (vec == 2) fn(double(), std::integral_constant<int, 2>()); else fn(double(), std::integral_constant<int, 1>());
    } else {
        if (vec == 4) fn(float(), std::integral_constant<int, 4>()); else fn(float(), std::integral_constant<int, 1>());
    }
}

}  // namespace pdehip
