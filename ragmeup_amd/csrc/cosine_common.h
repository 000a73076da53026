// cosine_common.h -- what the fp64 cosine units share (semantic.hip: adjacent rows; provenance.hip: member rows against one or two anchors):
// the lane's fragment of a row, the fixed-order fp64 sums and the fields of the calling thread's workspace (gfx950 only; its buffers and the
// error path are rmu_host.h's).
//
// The order of every sum is fixed by the element index alone: element e belongs to lane (e >> 2) & 63; a lane adds its elements in ascending
// order, starting from +0.0 (fma(a, b, acc) rounds once, like acc + exact product: an fp64 product of two fp32 values is exact); the 64 lane
// sums are folded by an xor butterfly over 32, 16, 8, 4, 2, 1 (every lane ends with the same bits).  A lane holds the elements
// 4 * (lane + 64 j) .. + 3, j < NJ, of a row as NJ float4 registers (NJ * 256 >= dim; elements past dim are +0.0 and add nothing), so a sum has
// the same bits in every instantiation that is wide enough and on either load path.
// Everything here has internal linkage: each unit has its own thread-local workspace.
#pragma once
#include <cstring>
#include <string>

#include "../../include/rmu.h"
#include "rmu_common.h"
#include "rmu_host.h"

namespace {

// the lane's NJ groups of four elements of one row; elements at or past dim are +0.0.  VEC: 16-byte loads (base 16-byte aligned, stride a
// multiple of 4 floats) for every group of four that lies inside the row; the last, partial group and the whole row otherwise take 4-byte loads
template <int NJ, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int dim, int lane, f32x4 (&f)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 4 * (lane + 64 * j);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (VEC && e + 4 <= dim) {
            v = *reinterpret_cast<const f32x4*>(row + e);
        } else {
            if (e < dim) v.x = row[e];
            if (e + 1 < dim) v.y = row[e + 1];
            if (e + 2 < dim) v.z = row[e + 2];
            if (e + 3 < dim) v.w = row[e + 3];
        }
        f[j] = v;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int NJ>
__device__ __forceinline__ double lane_norm2(const f32x4 (&f)[NJ]) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = (double)f[j][c];
            acc = __builtin_fma(v, v, acc);
        }
    return acc;
}

// the calling thread's workspace of one unit: the uploaded rows, the results, a small table, and the pinned buffer the host side of a call
// goes through.  Only a call that drains its stream uses it, so nothing of it is ever in flight between two calls (and its members free
// themselves at thread exit: nothing has an order)
struct CosCtx {
    RmuDevBuf in, out, tab;
    RmuPinBuf pin{8192};
};

}  // namespace
