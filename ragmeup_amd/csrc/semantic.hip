// semantic.hip -- cosine distance of every pair of ADJACENT rows of one fp32 matrix, in fp64, on the device (gfx950 only).
//
// Serves: langchain_experimental's SemanticChunker(self.embeddings, ...) (server/RAGHelper.py:329-349): the splitter embeds one window per
// sentence and needs ONE number per adjacent pair of windows, 1 - cosine_similarity(e[i], e[i + 1]).  The embeddings are on the device already
// (MI355XEmbeddings.embed_documents_device); this unit turns [n, dim] fp32 into [n - 1] fp64 there, so n - 1 doubles cross the bus instead of
// n * dim floats turned into Python lists (ragmeup_amd/chunker.py is the host half).
//
//   out[i] = 1 - dot / (sqrt(|a|^2) * sqrt(|b|^2)),  a = x[i], b = x[i + 1];  a quotient that is NaN or +-Inf counts as 0 (out = 1.0).
//
// dot, |a|^2 and |b|^2 are fp64 sums of fp64 products of fp32 values.  Such a product is exact (24 + 24 significant bits, exponents far inside
// fp64's range), so a sum depends on nothing but the ORDER of its additions, and that order is fixed by the element index alone:
//   element e belongs to lane (e >> 2) & 63; a lane adds its elements in ascending order, starting from +0.0 (fma(a, b, acc) rounds once, like
//   acc + exact product); the 64 lane sums are folded by an xor butterfly over 32, 16, 8, 4, 2, 1 (every lane ends with the same bits).
// out[i] therefore has the same bits whatever n, wherever the pair sits in the call, whichever load path its alignment selects and whichever
// instantiation serves its width: the tests compare rows passed alone against the same rows inside a larger call, bit for bit.
//
// Kernel (adjacent_cosine_kernel<NJ, VEC>): a wave owns kWavePairs consecutive pairs, i.e. kWavePairs + 1 consecutive rows.  A lane holds the
// elements 4 * (lane + 64 j) .. + 3, j < NJ, of a row as NJ float4 registers (NJ * 256 >= dim; elements past dim are zeros and add nothing).
// Row r's fragment and its |x_r|^2 stay in registers while row r + 1 is used, and row r + 2 is already in flight: a row is fetched once per
// wave, plus the one row two neighbouring runs share.  VEC: 16-byte loads (base 16-byte aligned, stride a multiple of 4 floats) for every
// group of four that lies inside the row; the last, partial group and the whole row otherwise take 4-byte loads.  Columns dim .. stride - 1
// are never read.  No LDS, no atomics, no scratch.
#include <cmath>

#include "cosine_common.h"      // load_row, wave_sum, lane_norm2, the thread's workspace (CosCtx), COS_TRY / cos_fail

namespace {

constexpr int kBlock = 256;                                  // 4 waves
constexpr int kWavePairs = 16;                               // pairs one wave owns (ragmeup_amd/_native.py: ADJ_COS_WAVE_PAIRS)
constexpr int kBlockPairs = kWavePairs * (kBlock / 64);      // pairs one workgroup owns (ADJ_COS_WG_PAIRS)

template <int NJ, bool VEC>
__global__ __launch_bounds__(kBlock) void adjacent_cosine_kernel(const float* __restrict__ x, int64_t n_pairs, int dim, int64_t stride,
                                                                 double* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t p0 = wave * kWavePairs;
    if (p0 >= n_pairs) return;                                // (wave-uniform)
    const int cnt = (int)(n_pairs - p0 < kWavePairs ? n_pairs - p0 : kWavePairs);
    const float* row = x + p0 * stride;                       // rows p0 .. p0 + cnt <= n_pairs = n - 1

    f32x4 a[NJ], b[NJ], c[NJ];
    load_row<NJ, VEC>(row, dim, lane, a);
    load_row<NJ, VEC>(row + stride, dim, lane, b);
    double na = wave_sum(lane_norm2<NJ>(a));
    for (int i = 0; i < cnt; ++i) {
        // b = row p0 + i + 1.  The row after it goes in flight before this pair's arithmetic
        if (i + 1 < cnt) {
            load_row<NJ, VEC>(row + (int64_t)(i + 2) * stride, dim, lane, c);
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j) c[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        double dot = 0.0, nb = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double va = (double)a[j][k], vb = (double)b[j][k];
                dot = __builtin_fma(va, vb, dot);
                nb = __builtin_fma(vb, vb, nb);
            }
        dot = wave_sum(dot);
        nb = wave_sum(nb);
        if (lane == 0) {
            double sim = dot / (sqrt(na) * sqrt(nb));
            if (!(fabs(sim) <= 1.7976931348623157e308)) sim = 0.0;      // NaN or +-Inf: a zero row, a NaN / Inf element
            out[p0 + i] = 1.0 - sim;
        }
        na = nb;
#pragma unroll
        for (int j = 0; j < NJ; ++j) { a[j] = b[j]; b[j] = c[j]; }
    }
}

template <int NJ>
void launch_nj(bool vec, unsigned grid, hipStream_t s, const float* x, int64_t n_pairs, int dim, int64_t stride, double* out) {
    if (vec) hipLaunchKernelGGL((adjacent_cosine_kernel<NJ, true>), dim3(grid), dim3(kBlock), 0, s, x, n_pairs, dim, stride, out);
    else hipLaunchKernelGGL((adjacent_cosine_kernel<NJ, false>), dim3(grid), dim3(kBlock), 0, s, x, n_pairs, dim, stride, out);
}

// x, out: device.  n_pairs >= 1 and the grid fits (checked by the entry point)
void launch(const float* x, int64_t n_pairs, int dim, int64_t stride, double* out, hipStream_t s) {
    const bool vec = ((uintptr_t)x & 15) == 0 && (stride & 3) == 0;
    const unsigned grid = (unsigned)((n_pairs + kBlockPairs - 1) / kBlockPairs);
    const int nj = (dim + 255) / 256;
    if (nj <= 1) launch_nj<1>(vec, grid, s, x, n_pairs, dim, stride, out);
    else if (nj <= 2) launch_nj<2>(vec, grid, s, x, n_pairs, dim, stride, out);
    else if (nj <= 4) launch_nj<4>(vec, grid, s, x, n_pairs, dim, stride, out);
    else if (nj <= 8) launch_nj<8>(vec, grid, s, x, n_pairs, dim, stride, out);
    else launch_nj<12>(vec, grid, s, x, n_pairs, dim, stride, out);
}

// the calling thread's workspace: the uploaded rows, the distances and their pinned landing place.  Only a call that drains its stream uses it
// (a call with a caller stream and device buffers on both sides touches none of it), so nothing of it is ever in flight between two calls
thread_local CosCtx g_ctx;

}  // namespace

extern "C" int rmu_adjacent_cosine(const float* x, int64_t n, int dim, int64_t stride, unsigned flags, double* out, uint64_t hip_stream) {
    RMU_ENTRY();
    if (!x || !out) return rmu_fail(RMU_E_INVALID, "rmu_adjacent_cosine: null pointer");
    if (flags & ~(RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE))
        return rmu_fail(RMU_E_INVALID, "rmu_adjacent_cosine: flags other than RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE");
    if (dim < 1 || dim > RMU_MAX_DIM_WIDE) return rmu_fail(RMU_E_INVALID, "rmu_adjacent_cosine: 1 <= dim <= RMU_MAX_DIM_WIDE (3072)");
    if (stride < dim) return rmu_fail(RMU_E_INVALID, "rmu_adjacent_cosine: stride must be >= dim");
    if (n < 1) return rmu_fail(RMU_E_INVALID, "rmu_adjacent_cosine: n must be >= 1");
    // the matrix in bytes and the grid (one workgroup per kBlockPairs pairs) must stay representable
    if (n > (int64_t)0x7FFFFFFFll * kBlockPairs || stride > INT64_MAX / 4 / n)
        return rmu_fail(RMU_E_INVALID, "rmu_adjacent_cosine: n * stride is too large");
    if (n == 1) return RMU_OK;                                  // no pair: nothing is written, nothing is launched
    const bool in_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE;
    const int64_t n_pairs = n - 1;

    CosCtx& c = g_ctx;
    hipStream_t s = nullptr;
    int rc = rmu_thread_stream_((hipStream_t)hip_stream, &s);
    if (rc) return rc;
    const size_t in_bytes = ((size_t)n_pairs * (size_t)stride + (size_t)dim) * sizeof(float);      // (the last row's pad columns are not touched)
    const size_t out_bytes = (size_t)n_pairs * sizeof(double);
    if (!in_dev) RMU_HIP_TRY(c.in.ensure(in_bytes));
    if (!out_dev) {
        RMU_HIP_TRY(c.out.ensure(out_bytes));
        if (c.pin.ensure(out_bytes) != RMU_OK) return rmu_fail(RMU_E_OOM, "rmu_adjacent_cosine: pinned result buffer");
    }
    const bool drained = !hip_stream || !out_dev || !in_dev;
    const float* dx = x;
    double* dout = out;
    hipError_t e = hipSuccess;
    if (!in_dev) {
        e = hipMemcpyAsync(c.in.p, x, in_bytes, hipMemcpyHostToDevice, s);
        dx = (const float*)c.in.p;
    }
    if (e == hipSuccess) {
        if (!out_dev) dout = (double*)c.out.p;
        launch(dx, n_pairs, dim, stride, dout, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !out_dev) e = hipMemcpyAsync(c.pin.p, dout, out_bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) {                                      // nothing of a failed call stays in flight on the thread's workspace
        (void)hipStreamSynchronize(s);
        rmu_thread_finished_(s, true);
        return rmu_fail(RMU_E_HIP, std::string("rmu_adjacent_cosine: ") + hipGetErrorString(e));
    }
    if (drained) {
        e = hipStreamSynchronize(s);
        rmu_thread_finished_(s, true);
        if (e != hipSuccess) return rmu_fail(RMU_E_HIP, std::string("rmu_adjacent_cosine: ") + hipGetErrorString(e));
        if (!out_dev) memcpy(out, c.pin.p, out_bytes);
        return RMU_OK;
    }
    // left in flight on the caller's stream: it touched none of the thread's workspaces, so the thread's pending state stays as it was and
    // its next call on another stream is not ordered behind this kernel
    return RMU_OK;
}
