// rmu_compact.hip -- row moves of rmu_index_compact (include/rmu.h): the live rows of one array of the index are gathered to the
// front, in order, and everything past the last live row is reset to what a fresh index holds there.
//
// Serves: server.py:353-385 (POST /delete) + RAGHelper.py:518-538 (a re-uploaded file's chunks replace their old rows): without it
// every tombstone keeps its fp32 row, its fp16 screening image and its norm in HBM for the life of the process, and every scan reads it.
//
// The gather is a pure streaming copy: 16-byte pieces, (row, piece) mapped flatly onto threads so a 1536-B row is 96 consecutive
// lanes and no wave idles at a row's end; the source is read once (non-temporal loads), the destination is written with plain stores
// (MI355X: 6.0-6.2 TB/s for 256 contiguous bytes per wave-instruction).
#include <algorithm>

#include "rmu_common.h"
#include "../../include/rmu.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// dst row j (j in [0, rows)) <- src row src_rows[j]; PER_ROW elements of T per row.  U pieces per thread, all loads issued before
// the first store.
template <typename T, int PER_ROW, int U>
__global__ __launch_bounds__(256) void k_compact_rows(const T* __restrict__ src, T* __restrict__ dst, const u32* __restrict__ src_rows,
                                                      int64_t rows) {
    const int64_t total = rows * PER_ROW;
    const int64_t i0 = (int64_t)blockIdx.x * (256 * U) + threadIdx.x;
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * 256;
        if (i < total) {
            const int64_t r = i / PER_ROW;
            const int64_t p = i - r * PER_ROW;
            v[u] = __builtin_nontemporal_load(src + (int64_t)src_rows[r] * PER_ROW + p);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * 256;
        if (i < total) dst[i] = v[u];
    }
}

// the same for rows of any whole number of 16-byte pieces (per_row at run time): the wide rows of scan_wide.hip, 64 to 3072 floats
template <int U>
__global__ __launch_bounds__(256) void k_compact_rows_any(const u32x4* __restrict__ src, u32x4* __restrict__ dst, const u32* __restrict__ src_rows,
                                                          int64_t rows, int per_row) {
    const int64_t total = rows * per_row;
    const int64_t i0 = (int64_t)blockIdx.x * (256 * U) + threadIdx.x;
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * 256;
        if (i < total) {
            const int64_t r = i / per_row;
            const int64_t p = i - r * per_row;
            v[u] = __builtin_nontemporal_load(src + (int64_t)src_rows[r] * per_row + p);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * 256;
        if (i < total) dst[i] = v[u];
    }
}

template <typename T, int PER_ROW>
static hipError_t launch_rows(const void* src, void* dst, const u32* src_rows, int64_t rows, hipStream_t s) {
    constexpr int U = 4;
    const int64_t total = rows * PER_ROW;
    const int64_t grid = (total + 256 * U - 1) / (256 * U);
    if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_compact_rows<T, PER_ROW, U>), dim3((unsigned)grid), dim3(256), 0, s, (const T*)src, (T*)dst, src_rows, rows);
    return hipGetLastError();
}

// rows of row_bytes: 768 / 1536 / 3072 (fp32 rows of dpad 192 / 384 / 768; 768 is also the fp16 screening image), 4 (L2 norms), or any
// other multiple of 256 (the wide rows: dpad is a multiple of 64 floats)
static hipError_t gather(const void* src, void* dst, int64_t row_bytes, const u32* src_rows, int64_t rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    switch (row_bytes) {
        case 768: return launch_rows<u32x4, 48>(src, dst, src_rows, rows, s);
        case 1536: return launch_rows<u32x4, 96>(src, dst, src_rows, rows, s);
        case 3072: return launch_rows<u32x4, 192>(src, dst, src_rows, rows, s);
        case 4: return launch_rows<float, 1>(src, dst, src_rows, rows, s);
        default: break;
    }
    if (row_bytes % 256 != 0 || row_bytes > (int64_t)RMU_MAX_DIM_WIDE * 4) return hipErrorInvalidValue;
    constexpr int U = 4;
    const int per_row = (int)(row_bytes / 16);
    const int64_t grid = (rows * per_row + 256 * U - 1) / (256 * U);
    if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_compact_rows_any<U>, dim3((unsigned)grid), dim3(256), 0, s, (const u32x4*)src, (u32x4*)dst, src_rows, rows, per_row);
    return hipGetLastError();
}

hipError_t rmu_compact_array(void** base, int64_t row_bytes, int fill, int64_t n_old, int64_t n_live, int64_t first, const u32* src_rows,
                             int64_t alloc_rows, void* staging, size_t staging_bytes, hipStream_t s) {
    char* old = (char*)*base;
    const int64_t nmove = n_live - first;
    hipError_t e;
    if (alloc_rows > 0) {
        char* nb = nullptr;
        if ((e = hipMalloc((void**)&nb, (size_t)alloc_rows * row_bytes)) != hipSuccess) { (void)hipGetLastError(); return e; }
        if ((e = hipMemsetAsync(nb + n_live * row_bytes, fill, (size_t)(alloc_rows - n_live) * row_bytes, s)) != hipSuccess ||
            (first > 0 && (e = hipMemcpyAsync(nb, old, (size_t)first * row_bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess) ||
            (e = gather(old, nb + first * row_bytes, row_bytes, src_rows, nmove, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess) {
            (void)hipStreamSynchronize(s);
            (void)rmu_free(nb);
            return e;
        }
        (void)rmu_free(old);
        *base = nb;
        return hipSuccess;
    }
    // in place: chunk [j0, j0 + c) gathers its sources (rows >= j0, since src_rows[j - first] >= j, none of them written by an earlier
    // chunk) into the staging buffer, then lands there; rows [n_live, n_old) are reset last
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(staging_bytes / (size_t)row_bytes));
    if (nmove > 0 && !staging) return hipErrorInvalidValue;
    for (int64_t j0 = first; j0 < n_live; j0 += chunk) {
        const int64_t c = std::min<int64_t>(chunk, n_live - j0);
        if ((e = gather(old, staging, row_bytes, src_rows + (j0 - first), c, s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(old + j0 * row_bytes, staging, (size_t)c * row_bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    }
    if (n_old > n_live) return hipMemsetAsync(old + n_live * row_bytes, fill, (size_t)(n_old - n_live) * row_bytes, s);
    return hipSuccess;
}
