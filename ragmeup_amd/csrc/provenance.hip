// provenance.hip -- similarity provenance: how much of an answer each retrieved document accounts for, in fp64, on the device (gfx950 only).
//
// Serves: DocumentSimilarityAttribution.compute_similarity (server/provenance.py:164-202, provenance_method=similarity; called once per /chat
// request, RAGHelper_local.py:294-295): the answer, the query and the n retrieved documents are embedded, and every document gets
//   s_i = cos(doc_i, answer), or (cos(doc_i, answer) + cos(doc_i, query)) / 2 with the query included;  T = s_0 + s_1 + ...;
//   score_i = s_i / T if T > 0, else s_i.
// The embeddings are on the device already (the encoder's output); this unit turns "one anchor row or two, n member rows" into n doubles
// there, for any number of requests (groups) in one launch (ragmeup_amd/provenance.py is the host half).
//
// Arithmetic (cosine_common.h): dot, |a|^2 and |b|^2 are fp64 sums of exact fp64 products in an order fixed by the element index alone;
// sim = dot / (sqrt(|a|^2) * sqrt(|b|^2)), and a quotient that is NaN or +-Inf (a zero row, a NaN / Inf element) counts as 0;
// s = sim_a, or (sim_a + sim_q) / 2; T is accumulated from +0.0 in document order; out = s / T (a true division) when T > 0, else s.
// Nothing depends on where a group or its rows sit in the call, on the load path the alignment selects or on the instantiation that serves
// the width: the tests compare a group passed alone against the same group inside a larger call, bit for bit.
//
// Kernel (attribution_kernel<NJ, VEC>): one wave per group, four waves per workgroup.  The answer's fragment, the query's (zeros without one)
// and both squared norms stay in registers as NJ float4 per lane; the group's document rows stream past them, the next row in flight before
// the current row's arithmetic.  Lane 0 writes the similarities and s_i, keeps T, and, when T > 0, divides what it wrote itself (the same
// lane: program order, no fence).  Rows may be shared between groups and may coincide with an anchor: rows are only read.  No LDS, no atomics,
// no scratch.
#include <cmath>

#include "cosine_common.h"      // load_row, wave_sum, lane_norm2, the thread's workspace (CosCtx), COS_TRY / cos_fail
#include "rmu_internal.h"      // rmu_attribution_check_ / _dev_: the prototypes bert.hip calls them by

namespace {

constexpr int kBlock = 256;                                  // 4 waves = 4 groups
constexpr int kTab = 5;                                      // device table, int32 per group: answer row, query row (-1), first row, rows, first output

__device__ __forceinline__ double finite_or_zero(double v) {
    return fabs(v) <= 1.7976931348623157e308 ? v : 0.0;       // NaN or +-Inf: a zero row, a NaN / Inf element
}

template <int NJ, bool VEC>
__global__ __launch_bounds__(kBlock) void attribution_kernel(const float* __restrict__ x, int dim, int64_t stride, const int* __restrict__ tab,
                                                             int n_groups, double* out_scores, double* out_sims) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int g = (int)blockIdx.x * (kBlock / 64) + (int)(threadIdx.x >> 6);
    if (g >= n_groups) return;                                // (wave-uniform)
    const int* t = tab + (int64_t)kTab * g;
    const int row_a = t[0], row_q = t[1], first = t[2], cnt = t[3], out0 = t[4];
    if (cnt <= 0) return;
    const bool has_q = row_q >= 0;

    f32x4 a[NJ], q[NJ], b[NJ], c[NJ];
    load_row<NJ, VEC>(x + (int64_t)row_a * stride, dim, lane, a);
    if (has_q) {
        load_row<NJ, VEC>(x + (int64_t)row_q * stride, dim, lane, q);
    } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j) q[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* row = x + (int64_t)first * stride;           // rows first .. first + cnt - 1 < n
    load_row<NJ, VEC>(row, dim, lane, b);
    const double na = wave_sum(lane_norm2<NJ>(a));
    const double nq = wave_sum(lane_norm2<NJ>(q));
    double total = 0.0;
    for (int i = 0; i < cnt; ++i) {
        // b = row first + i.  The row after it goes in flight before this row's arithmetic
        if (i + 1 < cnt) {
            load_row<NJ, VEC>(row + (int64_t)(i + 1) * stride, dim, lane, c);
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j) c[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        double da = 0.0, dq = 0.0, nb = 0.0;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double va = (double)a[j][k], vq = (double)q[j][k], vb = (double)b[j][k];
                da = __builtin_fma(vb, va, da);
                dq = __builtin_fma(vb, vq, dq);
                nb = __builtin_fma(vb, vb, nb);
            }
        da = wave_sum(da);
        dq = wave_sum(dq);
        nb = wave_sum(nb);
        if (lane == 0) {
            const double rb = sqrt(nb);
            const double sim_a = finite_or_zero(da / (rb * sqrt(na)));
            const double sim_q = has_q ? finite_or_zero(dq / (rb * sqrt(nq))) : 0.0;
            const double s = has_q ? (sim_a + sim_q) / 2 : sim_a;
            total = total + s;
            out_scores[out0 + i] = s;
            if (out_sims) {
                out_sims[2 * (int64_t)(out0 + i)] = sim_a;
                out_sims[2 * (int64_t)(out0 + i) + 1] = sim_q;
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = c[j];
    }
    // the division reads back what this lane wrote
    if (lane == 0 && total > 0.0)
        for (int i = 0; i < cnt; ++i) out_scores[out0 + i] = out_scores[out0 + i] / total;
}

template <int NJ>
void launch_nj(bool vec, unsigned grid, hipStream_t s, const float* x, int dim, int64_t stride, const int* tab, int n_groups, double* out_scores,
               double* out_sims) {
    if (vec) hipLaunchKernelGGL((attribution_kernel<NJ, true>), dim3(grid), dim3(kBlock), 0, s, x, dim, stride, tab, n_groups, out_scores, out_sims);
    else hipLaunchKernelGGL((attribution_kernel<NJ, false>), dim3(grid), dim3(kBlock), 0, s, x, dim, stride, tab, n_groups, out_scores, out_sims);
}

// everything device; n_groups >= 1
void launch(const float* x, int dim, int64_t stride, const int* tab, int n_groups, double* out_scores, double* out_sims, hipStream_t s) {
    const bool vec = ((uintptr_t)x & 15) == 0 && (stride & 3) == 0;
    const unsigned grid = (unsigned)((n_groups + kBlock / 64 - 1) / (kBlock / 64));
    const int nj = (dim + 255) / 256;
    if (nj <= 1) launch_nj<1>(vec, grid, s, x, dim, stride, tab, n_groups, out_scores, out_sims);
    else if (nj <= 2) launch_nj<2>(vec, grid, s, x, dim, stride, tab, n_groups, out_scores, out_sims);
    else if (nj <= 4) launch_nj<4>(vec, grid, s, x, dim, stride, tab, n_groups, out_scores, out_sims);
    else if (nj <= 8) launch_nj<8>(vec, grid, s, x, dim, stride, tab, n_groups, out_scores, out_sims);
    else launch_nj<12>(vec, grid, s, x, dim, stride, tab, n_groups, out_scores, out_sims);
}

// the calling thread's workspace: the uploaded rows, the group table, the results and the pinned buffer the table and the host results go
// through.  Every call drains its stream, so nothing of it is ever in flight between two calls
thread_local CosCtx g_ctx;

// every argument but the encoder's; *total = sum of n_docs.  No HIP call
int check_args(const std::string& w, const void* x, int64_t n, int dim, int64_t stride, const int32_t* groups, int n_groups, unsigned flags,
               const void* out_scores, int64_t* total) {
    if (!x || !groups || !out_scores) return rmu_fail(RMU_E_INVALID, w + ": null pointer");
    if (flags & ~(RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE)) return rmu_fail(RMU_E_INVALID, w + ": flags other than RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE");
    if (dim < 1 || dim > RMU_MAX_DIM_WIDE) return rmu_fail(RMU_E_INVALID, w + ": 1 <= dim <= RMU_MAX_DIM_WIDE (3072)");
    if (stride < dim) return rmu_fail(RMU_E_INVALID, w + ": stride must be >= dim");
    if (n < 1) return rmu_fail(RMU_E_INVALID, w + ": n must be >= 1");
    if (stride > INT64_MAX / 4 / n) return rmu_fail(RMU_E_INVALID, w + ": n * stride is too large");
    if (n_groups < 0) return rmu_fail(RMU_E_INVALID, w + ": n_groups must be >= 0");
    int64_t sum = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int32_t* t = groups + 4 * (int64_t)g;
        const std::string at = w + ": group " + std::to_string(g);
        if (t[0] < 0 || t[0] >= n) return rmu_fail(RMU_E_INVALID, at + ": the answer row is outside [0, n)");
        if (t[1] < -1 || t[1] >= n) return rmu_fail(RMU_E_INVALID, at + ": the query row is outside [0, n) and not -1");
        if (t[3] < 0) return rmu_fail(RMU_E_INVALID, at + ": n_docs must be >= 0");
        if (t[2] < 0 || t[2] >= n || (int64_t)t[2] + t[3] > n) return rmu_fail(RMU_E_INVALID, at + ": the document rows are outside [0, n)");
        sum += t[3];
        if (sum > INT32_MAX) return rmu_fail(RMU_E_INVALID, w + ": the sum of n_docs does not fit in an int32");
    }
    *total = sum;
    return RMU_OK;
}

// checked arguments, total >= 1.  Drains its stream
int attribution_on(const std::string& w, const float* x, int64_t n, int dim, int64_t stride, const int32_t* groups, int n_groups, unsigned flags,
                   int64_t total, double* out_scores, double* out_sims, hipStream_t user) {
    const bool in_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE;
    CosCtx& c = g_ctx;
    hipStream_t s = nullptr;
    int rc = rmu_thread_stream_(user, &s);
    if (rc) return rc;
    const size_t in_bytes = ((size_t)(n - 1) * (size_t)stride + (size_t)dim) * sizeof(float);      // (the last row's pad columns are not touched)
    const size_t tab_bytes = ((size_t)n_groups * kTab * sizeof(int32_t) + 7) & ~(size_t)7;
    const size_t score_bytes = (size_t)total * sizeof(double);
    const size_t out_bytes = score_bytes * (out_sims ? 3 : 1);                                      // scores [total] | sims [total, 2]
    if (!in_dev) RMU_HIP_TRY(c.in.ensure(in_bytes));
    RMU_HIP_TRY(c.tab.ensure(tab_bytes));
    if (!out_dev) RMU_HIP_TRY(c.out.ensure(out_bytes));
    if (c.pin.ensure(tab_bytes + (out_dev ? 0 : out_bytes)) != RMU_OK) return rmu_fail(RMU_E_OOM, w + ": pinned buffer");
    int32_t* tab = (int32_t*)c.pin.p;
    int32_t out0 = 0;
    for (int g = 0; g < n_groups; ++g) {
        memcpy(tab + (size_t)kTab * g, groups + 4 * (size_t)g, 4 * sizeof(int32_t));
        tab[(size_t)kTab * g + 4] = out0;
        out0 += groups[4 * (size_t)g + 3];
    }
    char* land = c.pin.p + tab_bytes;
    const float* dx = x;
    double* d_scores = out_scores;
    double* d_sims = out_sims;
    hipError_t e = hipMemcpyAsync(c.tab.p, tab, tab_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !in_dev) {
        e = hipMemcpyAsync(c.in.p, x, in_bytes, hipMemcpyHostToDevice, s);
        dx = (const float*)c.in.p;
    }
    if (e == hipSuccess) {
        if (!out_dev) {
            d_scores = (double*)c.out.p;
            d_sims = out_sims ? d_scores + total : nullptr;
        }
        launch(dx, dim, stride, (const int*)c.tab.p, n_groups, d_scores, d_sims, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !out_dev) e = hipMemcpyAsync(land, d_scores, out_bytes, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);              // always: the table went through the thread's pinned buffer
    rmu_thread_finished_(s, true);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return rmu_fail(RMU_E_HIP, w + ": " + hipGetErrorString(e));
    if (!out_dev) {
        memcpy(out_scores, land, score_bytes);
        if (out_sims) memcpy(out_sims, land + score_bytes, 2 * score_bytes);
    }
    return RMU_OK;
}

}  // namespace

extern "C" int rmu_attribution(const float* x, int64_t n, int dim, int64_t stride, const int32_t* groups, int n_groups, unsigned flags,
                               double* out_scores, double* out_sims, uint64_t hip_stream) {
    RMU_ENTRY();
    int64_t total = 0;
    const int rc = check_args("rmu_attribution", x, n, dim, stride, groups, n_groups, flags, out_scores, &total);
    if (rc) return rc;
    if (total == 0) return RMU_OK;                              // no document: nothing is written, nothing is launched
    return attribution_on("rmu_attribution", x, n, dim, stride, groups, n_groups, flags, total, out_scores, out_sims, (hipStream_t)hip_stream);
}

// bert.hip (rmu_bert_attribute): the table against `n` encoder rows before the forward ...
extern "C" int rmu_attribution_check_(const char* who, int64_t n, int dim, const int32_t* groups, int n_groups, const double* out_scores,
                                      int64_t* total) {
    return check_args(who, who /* (x is the encoder's) */, n, dim, dim, groups, n_groups, 0, out_scores, total);
}
// ... and the kernel behind it: DEVICE rows on the encoder's stream, HOST results; drains the stream
extern "C" int rmu_attribution_dev_(const char* who, const float* x_dev, int64_t n, int dim, int64_t stride, const int32_t* groups, int n_groups,
                                    int64_t total, double* out_scores, double* out_sims, void* hip_stream) {
    RMU_ENTRY();
    if (!x_dev || !hip_stream) return rmu_fail(RMU_E_INVALID, std::string(who) + ": null pointer");
    return attribution_on(who, x_dev, n, dim, stride, groups, n_groups, RMU_F_Q_DEVICE, total, out_scores, out_sims, (hipStream_t)hip_stream);
}
