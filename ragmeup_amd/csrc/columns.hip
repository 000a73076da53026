// columns.hip -- metadata columns in HBM and the row lists of a filtered search built on the device (include/rmu.h, "metadata columns").
//
// Reference call sites served (server/ = the reference's server directory):
//   rmu_columns_select / rmu_index_search_where   RAGHelper.py:497-499 with search_kwargs (Milvus col.search(expr='source == "a.pdf"') /
//                                                 PGVector filter={"source": "a.pdf"}): the part IN FRONT of the gathered scan -- which rows
//                                                 does the condition name -- that ragmeup_amd/vectorstore.py answers with a Python walk over
//                                                 every record after each upload or delete (server.py:150-183, 353-385)
//   rmu_columns_append / rmu_columns_compact      RAGHelper.py:518-538 (upload), server.py:353-385 (delete + re-upload cycle)
//
// Layout.  One int32 code per (row, field): the host numbers the values of each field, the library sees codes >= 0 only.  The host master
// copy is field-major (one vector per field); the device image is field-major as well -- field f is the int32 array img + f * cap_rows,
// cap_rows a multiple of 1024, so a lane's four consecutive rows are one aligned 16-byte load.  The image follows the master lazily: its
// first d_len rows are current, the tail is uploaded by the next selection under the exclusive lock, and it is re-allocated (and uploaded
// whole) only when the rows no longer fit.
//
// Selection = an order-preserving stream compaction, three passes over (tiles x named selections):
//   1. col_count_kernel   a workgroup takes a tile of rows (default 4096 = 256 lanes x 16 rows, four dwordx4 loads per lane and field),
//                         evaluates the selection (a single code: a compare; a set: a binary search over the sorted codes in LDS), reduces
//                         the matches with __ballot + __popcll, one count per wave in LDS, one count per (selection, tile) in global memory;
//   2. col_scan_kernel    exclusive scan of a selection's tile counts (in place: tile offsets) and its total; the same kernel then scans
//                         the totals into list_ptr -- the n_sel + 1 numbers the host reads, through the pinned buffer, one synchronisation;
//   3. col_write_kernel   evaluates the selection again (the columns are 4 bytes per row and field; a kept match mask would be written and
//                         read back at 1 bit per row and selection for nothing) and every lane writes its int64 row ids at
//                         list base + tile offset + matches of earlier iterations + wave prefix + mbcnt lane prefix: ascending by construction.
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>
#include <new>
#include <cstring>

#include "rmu_common.h"
#include "rmu_host.h"
#include "../../include/rmu.h"

namespace {

constexpr int kBlock = 256;                  // lanes per workgroup (4 waves)
constexpr int kLaneRows = 4;                 // consecutive rows per lane and load (one dwordx4)
constexpr int kIterRows = kBlock * kLaneRows;
constexpr int kDefaultTileRows = 4096;       // 256 lanes x 16 rows
constexpr int kMaxTerms = 4;
constexpr int kMaxCodes = 1024;              // per selection, all terms together: 4 KiB of LDS
constexpr int kMaxFields = 8;
constexpr int kMaxSelections = 8192;

// one named selection as the kernels read it: term t tests column field[t] against codes[code_off[t] .. code_off[t] + n_codes[t])
struct ColSel {
    int32_t n_terms;
    int32_t field[kMaxTerms];
    int32_t code_off[kMaxTerms];
    int32_t n_codes[kMaxTerms];
    int32_t pad[3];
};
static_assert(sizeof(ColSel) == 64, "ColSel");

struct SelLds {
    ColSel d;
    int lo[kMaxTerms];            // where term t's codes start in `codes`
    int codes[kMaxCodes];
};

// the workgroup's selection into LDS (descriptor, then the codes of its terms laid end to end); ends with a barrier
__device__ __forceinline__ void sel_load(SelLds& L, const ColSel* __restrict__ sels, const int32_t* __restrict__ codes, int sel) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        L.d = sels[sel];
        int lo = 0;
        for (int t = 0; t < kMaxTerms; ++t) {
            L.lo[t] = lo;
            if (t < L.d.n_terms) lo += L.d.n_codes[t];
        }
    }
    __syncthreads();
    for (int t = 0; t < L.d.n_terms; ++t) {
        const int nc = L.d.n_codes[t], off = L.d.code_off[t], lo = L.lo[t];
        for (int i = tid; i < nc; i += kBlock)
            if (lo + i < kMaxCodes) L.codes[lo + i] = codes[off + i];
    }
    __syncthreads();
}

__device__ __forceinline__ unsigned member(const int* s, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo < n && s[lo] == v ? 1u : 0u;
}

// bit j = row r0 + j satisfies the selection; rows at or past `end` (the tile's end, itself <= the row count) never do.  r0 is a multiple
// of 4 and every field array holds a multiple of 1024 rows, so the 16-byte load of a lane with r0 < end stays inside its array.
__device__ __forceinline__ unsigned eval4(const SelLds& L, const int32_t* __restrict__ img, int64_t cap, int64_t r0, int64_t end) {
    if (r0 >= end) return 0u;
    unsigned m = 0xFu;
    for (int t = 0; t < L.d.n_terms; ++t) {
        const int4 v = *reinterpret_cast<const int4*>(img + (int64_t)L.d.field[t] * cap + r0);
        const int nc = L.d.n_codes[t];
        const int* s = L.codes + L.lo[t];
        unsigned mt;
        if (nc == 1) {
            const int c = s[0];
            mt = (v.x == c ? 1u : 0u) | (v.y == c ? 2u : 0u) | (v.z == c ? 4u : 0u) | (v.w == c ? 8u : 0u);
        } else {
            mt = member(s, nc, v.x) | (member(s, nc, v.y) << 1) | (member(s, nc, v.z) << 2) | (member(s, nc, v.w) << 3);
        }
        m &= mt;
    }
    const int64_t left = end - r0;
    if (left < kLaneRows) m &= (1u << (int)left) - 1u;
    return m;
}

// pass 1: counts[sel * n_tiles + tile] = rows of the tile that satisfy the selection.  grid (n_tiles, n_named)
__global__ __launch_bounds__(kBlock) void col_count_kernel(const int32_t* __restrict__ img, int64_t cap, int64_t n, int tile_rows,
                                                           const ColSel* __restrict__ sels, const int32_t* __restrict__ codes,
                                                           u32* __restrict__ counts, int n_tiles) {
    __shared__ SelLds L;
    __shared__ u32 wcnt[kBlock / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sel = blockIdx.y, tile = blockIdx.x;
    sel_load(L, sels, codes, sel);
    const int64_t tb = (int64_t)tile * tile_rows;
    const int64_t te = tb + tile_rows < n ? tb + tile_rows : n;
    const int iters = (int)((te - tb + kIterRows - 1) / kIterRows);
    u32 c = 0;                               // wave-uniform
    for (int it = 0; it < iters; ++it) {
        const unsigned m = eval4(L, img, cap, tb + (int64_t)it * kIterRows + tid * kLaneRows, te);
        c += __popcll(__ballot(m & 1u)) + __popcll(__ballot(m & 2u)) + __popcll(__ballot(m & 4u)) + __popcll(__ballot(m & 8u));
    }
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    if (tid == 0) counts[(size_t)sel * n_tiles + tile] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// pass 2: in-place exclusive scan of segment blockIdx.x of `data` (seg_len entries each), its total to totals[blockIdx.x].  One
// workgroup walks its segment 256 entries at a time with a running carry.
template <class T>
__global__ __launch_bounds__(kBlock) void col_scan_kernel(T* __restrict__ data, int64_t seg_len, int64_t* __restrict__ totals) {
    __shared__ T s[kBlock];
    const int tid = threadIdx.x;
    T* seg = data + (size_t)blockIdx.x * seg_len;
    T carry = 0;
    for (int64_t base = 0; base < seg_len; base += kBlock) {
        const int64_t i = base + tid;
        const T v = i < seg_len ? seg[i] : (T)0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < kBlock; d <<= 1) {
            const T add = tid >= d ? s[tid - d] : (T)0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (i < seg_len) seg[i] = carry + s[tid] - v;
        carry += s[kBlock - 1];
        __syncthreads();
    }
    if (tid == 0) totals[blockIdx.x] = (int64_t)carry;
}

// pass 3: the row ids.  offs = the scanned counts (tile offsets inside a list), list_ptr = the scanned totals (where list `sel` starts)
__global__ __launch_bounds__(kBlock) void col_write_kernel(const int32_t* __restrict__ img, int64_t cap, int64_t n, int tile_rows,
                                                           const ColSel* __restrict__ sels, const int32_t* __restrict__ codes,
                                                           const u32* __restrict__ offs, int n_tiles, const int64_t* __restrict__ list_ptr,
                                                           int64_t* __restrict__ out) {
    __shared__ SelLds L;
    __shared__ u32 wcnt[kBlock / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sel = blockIdx.y, tile = blockIdx.x;
    sel_load(L, sels, codes, sel);
    const int64_t tb = (int64_t)tile * tile_rows;
    const int64_t te = tb + tile_rows < n ? tb + tile_rows : n;
    const int iters = (int)((te - tb + kIterRows - 1) / kIterRows);
    const int64_t base = list_ptr[sel] + offs[(size_t)sel * n_tiles + tile];
    u32 run = 0;                             // matches of the iterations in front (uniform)
    for (int it = 0; it < iters; ++it) {
        const int64_t r0 = tb + (int64_t)it * kIterRows + tid * kLaneRows;
        const unsigned m = eval4(L, img, cap, r0, te);
        const u64 b0 = __ballot(m & 1u), b1 = __ballot(m & 2u), b2 = __ballot(m & 4u), b3 = __ballot(m & 8u);
        if (lane == 0) wcnt[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
        __syncthreads();
        u32 wp = 0, tot = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            const u32 v = wcnt[w];
            if (w < wave) wp += v;
            tot += v;
        }
        // matches of the lower lanes of this wave: mbcnt over each of the four ballots
        u32 lp = 0;
        lp = __builtin_amdgcn_mbcnt_hi((u32)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b0, lp));
        lp = __builtin_amdgcn_mbcnt_hi((u32)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b1, lp));
        lp = __builtin_amdgcn_mbcnt_hi((u32)(b2 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b2, lp));
        lp = __builtin_amdgcn_mbcnt_hi((u32)(b3 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b3, lp));
        int64_t pos = base + run + wp + lp;
        if (m & 1u) out[pos++] = r0;
        if (m & 2u) out[pos++] = r0 + 1;
        if (m & 4u) out[pos++] = r0 + 2;
        if (m & 8u) out[pos++] = r0 + 3;
        run += tot;
        __syncthreads();
    }
}

// the calling thread's scratch: the selections on their way in, the tile counts, list_ptr, the lists
struct Ctx {
    RmuDevBuf sels, counts, lptr, lists;
    RmuPinBuf pin{8192};          // [ColSel x n_named | codes] on the way in, then list_ptr [n_named + 1] on the way out
    // RMU_COLUMNS_TIMING (a tuning switch: tools/where_probe.py): events around passes 1 + 2 and around pass 3 of the thread's last selection
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float count_ms = -1.f, write_ms = -1.f;
    bool wrote = false;           // pass 3 of the last selection was timed
    bool ensure_events() {
        for (auto& e : ev)
            if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; (void)hipGetLastError(); return false; }
        return true;
    }
    ~Ctx() {
        if (rmu_runtime_down()) return;
        RMU_ENTRY();
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
thread_local Ctx g_ctx;

bool timing_on() {
    static const bool on = rmu_env("RMU_COLUMNS_TIMING") != nullptr;
    return on;
}

}  // namespace

// Lock order: the columns' lock first, then the index's.  rmu_index_search_where holds the columns' shared lock while it reads the index's size
// and while rmu_index_search_groups runs under the index's shared lock; nothing takes the two the other way round (the store appends to the
// index and to the columns one after the other, never one inside the other).  A call that ever writes both must take them in this order.
struct rmu_columns {
    int n_fields = 0;
    std::vector<int32_t> col[kMaxFields];      // host master, field-major
    int64_t n = 0;
    RmuDevBuf img;                             // device image: field f at img + f * cap_rows
    int64_t cap_rows = 0;
    int64_t d_len = 0;                         // rows of the image that are current
    int tile_rows = 0;                         // RMU_COLUMNS_OPT_TILE_ROWS (0 = default)
    std::shared_mutex mu;
};

extern "C" int rmu_columns_create(rmu_columns_t** out, int n_fields, int64_t capacity_hint) {
    if (!out) return rmu_fail(RMU_E_INVALID, "rmu_columns_create: out is null");
    if (n_fields < 1 || n_fields > kMaxFields) return rmu_fail(RMU_E_INVALID, "rmu_columns_create: n_fields must be in [1, 8]");
    if (capacity_hint < 0) return rmu_fail(RMU_E_INVALID, "rmu_columns_create: capacity_hint must be >= 0");
    rmu_columns* c = new (std::nothrow) rmu_columns();
    if (!c) return rmu_fail(RMU_E_OOM, "rmu_columns_create: out of memory");
    c->n_fields = n_fields;
    try {
        for (int f = 0; f < n_fields; ++f) c->col[f].reserve((size_t)capacity_hint);
    } catch (...) { delete c; return rmu_fail(RMU_E_OOM, "rmu_columns_create: out of memory"); }
    *out = c;
    return RMU_OK;
}

extern "C" int rmu_columns_free(rmu_columns_t* c) {
    RMU_ENTRY();
    if (!c) return RMU_OK;
    { std::unique_lock<std::shared_mutex> lk(c->mu); }      // selections end under the shared lock with their stream drained
    delete c;                                               // (~RmuDevBuf frees the image)
    return RMU_OK;
}

extern "C" int rmu_columns_size(rmu_columns_t* c, int64_t* n_rows, int* n_fields) {
    if (!c) return rmu_fail(RMU_E_INVALID, "rmu_columns_size: null handle");
    std::shared_lock<std::shared_mutex> lk(c->mu);
    if (n_rows) *n_rows = c->n;
    if (n_fields) *n_fields = c->n_fields;
    return RMU_OK;
}

extern "C" int rmu_columns_append(rmu_columns_t* c, const int32_t* codes, int64_t n, int64_t* first_row) {
    if (!c || n < 0 || (n > 0 && !codes)) return rmu_fail(RMU_E_INVALID, "rmu_columns_append: bad argument");
    const int nf = c->n_fields;
    for (int64_t i = 0; i < n * nf; ++i)
        if (codes[i] < 0)
            return rmu_fail(RMU_E_INVALID, "rmu_columns_append: a code is negative: row " + std::to_string(i / nf) + ", field " + std::to_string(i % nf));
    std::unique_lock<std::shared_mutex> lk(c->mu);
    if (c->n + n >= 0xFFFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_columns_append: row ids must fit 32 bits");
    try {
        for (int f = 0; f < nf; ++f) c->col[f].reserve((size_t)(c->n + n));      // every field first: a failure changes nothing
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_columns_append: out of memory"); }
    for (int f = 0; f < nf; ++f) {
        std::vector<int32_t>& v = c->col[f];
        v.resize((size_t)(c->n + n));
        int32_t* dst = v.data() + c->n;
        for (int64_t i = 0; i < n; ++i) dst[i] = codes[i * nf + f];
    }
    if (first_row) *first_row = c->n;
    c->n += n;
    return RMU_OK;
}

extern "C" int rmu_columns_compact(rmu_columns_t* c, const int64_t* old_to_new, int64_t map_len, int64_t* n_after) {
    if (!c || (map_len > 0 && !old_to_new)) return rmu_fail(RMU_E_INVALID, "rmu_columns_compact: null argument");
    std::unique_lock<std::shared_mutex> lk(c->mu);
    const int64_t n = c->n;
    if (map_len < n)
        return rmu_fail(RMU_E_INVALID, "rmu_columns_compact: the map holds " + std::to_string(map_len) + " entries, the columns " + std::to_string(n) + " rows");
    // the contract of rmu_index_compact's map: live rows keep their order and become 0 .. n_live-1
    int64_t live = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t m = old_to_new[r];
        if (m < 0) continue;
        if (m != live) return rmu_fail(RMU_E_INVALID, "rmu_columns_compact: the map does not keep the order of the rows: entry " + std::to_string(r));
        ++live;
    }
    if (live != n) {
        for (int f = 0; f < c->n_fields; ++f) {
            int32_t* v = c->col[f].data();
            for (int64_t r = 0; r < n; ++r)
                if (old_to_new[r] >= 0) v[old_to_new[r]] = v[r];
            c->col[f].resize((size_t)live);
        }
        c->n = live;
        c->d_len = 0;                                      // the next selection uploads the image again
    }
    if (n_after) *n_after = c->n;
    return RMU_OK;
}

extern "C" int rmu_columns_set_option(rmu_columns_t* c, int option, int64_t value) {
    if (!c) return rmu_fail(RMU_E_INVALID, "rmu_columns_set_option: null handle");
    if (option != RMU_COLUMNS_OPT_TILE_ROWS) return rmu_fail(RMU_E_INVALID, "rmu_columns_set_option: unknown option");
    if (value != 0 && (value < 64 || value > 16384 || (value & (value - 1))))
        return rmu_fail(RMU_E_INVALID, "rmu_columns_set_option: RMU_COLUMNS_OPT_TILE_ROWS must be 0 or a power of two in [64, 16384]");
    std::unique_lock<std::shared_mutex> lk(c->mu);
    c->tile_rows = (int)value;
    return RMU_OK;
}

// every limit of the flattened selections, without touching HIP (n_fields never changes after create)
static int check_selections(const std::string& w, int n_fields, const rmu_col_term* terms, int n_terms, const int32_t* codes, const int32_t* sel_ptr,
                            int n_sel) {
    if (n_sel < 1 || n_sel > kMaxSelections) return rmu_fail(RMU_E_INVALID, w + ": n_sel must be in [1, 8192]");
    if (!terms || !sel_ptr || n_terms < 1) return rmu_fail(RMU_E_INVALID, w + ": null terms / sel_ptr, or no term");
    if (sel_ptr[0] != 0 || sel_ptr[n_sel] != n_terms) return rmu_fail(RMU_E_INVALID, w + ": sel_ptr must run from 0 to n_terms");
    for (int g = 0; g < n_sel; ++g) {
        const std::string sg = w + ": selection " + std::to_string(g);
        const int nt = sel_ptr[g + 1] - sel_ptr[g];
        if (sel_ptr[g] < 0 || sel_ptr[g + 1] > n_terms || nt < 0) return rmu_fail(RMU_E_INVALID, sg + ": sel_ptr must be non-decreasing inside [0, n_terms]");
        if (nt == 0) return rmu_fail(RMU_E_INVALID, sg + " has no term");
        if (nt > kMaxTerms) return rmu_fail(RMU_E_INVALID, sg + " has " + std::to_string(nt) + " terms (at most 4)");
        int64_t total = 0;
        for (int t = sel_ptr[g]; t < sel_ptr[g + 1]; ++t) {
            const rmu_col_term& T = terms[t];
            if (T.field < 0 || T.field >= n_fields)
                return rmu_fail(RMU_E_INVALID, sg + ": field " + std::to_string(T.field) + " is outside [0, " + std::to_string(n_fields) + ")");
            if (T.codes_begin < 0 || T.codes_end < T.codes_begin) return rmu_fail(RMU_E_INVALID, sg + ": a term's code range is not a range");
            total += T.codes_end - T.codes_begin;
            if (total > kMaxCodes) return rmu_fail(RMU_E_INVALID, sg + " carries more than 1024 codes");
            if (T.codes_end > T.codes_begin && !codes) return rmu_fail(RMU_E_INVALID, sg + ": codes is null");
            for (int i = T.codes_begin; i < T.codes_end; ++i)
                if (codes[i] < 0 || (i > T.codes_begin && codes[i] <= codes[i - 1]))
                    return rmu_fail(RMU_E_INVALID, sg + ": the codes of a term must be >= 0 and strictly ascending");
        }
    }
    return RMU_OK;
}

// (exclusive lock held: no selection of this handle is in flight) bring the device image up to the master; drains s
static int upload_image(rmu_columns* c, hipStream_t s) {
    const int64_t n = c->n;
    if (n > c->cap_rows || !c->img.p) {
        const int64_t cap = (n + n / 4 + 1024 + 1023) / 1024 * 1024;
        c->d_len = 0;
        c->cap_rows = 0;
        RMU_HIP_TRY(c->img.ensure((size_t)cap * c->n_fields * sizeof(int32_t)));
        c->cap_rows = cap;
    }
    if (c->d_len < n)
        for (int f = 0; f < c->n_fields; ++f)
            RMU_HIP_TRY(hipMemcpyAsync((int32_t*)c->img.p + (int64_t)f * c->cap_rows + c->d_len, c->col[f].data() + c->d_len,
                                       (size_t)(n - c->d_len) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));          // (the host vectors are pageable)
    c->d_len = n;
    return RMU_OK;
}

// Passes 1 and 2 for the selections named[0 .. n_named) over the first n rows (shared lock held, image current): lp [n_named + 1] receives
// list_ptr; the stream is drained.  The tile offsets, the selections and list_ptr stay in the thread's scratch for write_lists.
static int count_lists(const std::string& w, rmu_columns* c, int64_t n, const rmu_col_term* terms, const int32_t* codes, const int32_t* sel_ptr,
                       const int* named, int n_named, hipStream_t s, int64_t* lp, int* tile_rows_out, int* n_tiles_out) {
    Ctx& x = g_ctx;
    const int tile_rows = c->tile_rows ? c->tile_rows : kDefaultTileRows;
    const int64_t n_tiles64 = (n + tile_rows - 1) / tile_rows;
    const int n_tiles = (int)n_tiles64;
    *tile_rows_out = tile_rows; *n_tiles_out = n_tiles;
    size_t n_codes = 0;
    for (int i = 0; i < n_named; ++i)
        for (int t = sel_ptr[named[i]]; t < sel_ptr[named[i] + 1]; ++t) n_codes += (size_t)(terms[t].codes_end - terms[t].codes_begin);
    const size_t b_sel = (size_t)n_named * sizeof(ColSel), b_in = b_sel + n_codes * sizeof(int32_t), b_lp = (size_t)(n_named + 1) * sizeof(int64_t);
    if (x.pin.ensure(b_in > b_lp ? b_in : b_lp)) return rmu_fail(RMU_E_OOM, w + ": pinned staging buffer");
    RMU_HIP_TRY(x.sels.ensure(b_in));
    RMU_HIP_TRY(x.counts.ensure((size_t)n_named * n_tiles * sizeof(u32)));
    RMU_HIP_TRY(x.lptr.ensure(b_lp));
    ColSel* hs = (ColSel*)x.pin.p;
    int32_t* hc = (int32_t*)(x.pin.p + b_sel);
    int off = 0;
    for (int i = 0; i < n_named; ++i) {
        ColSel d{};
        const int t0 = sel_ptr[named[i]];
        d.n_terms = sel_ptr[named[i] + 1] - t0;
        for (int t = 0; t < d.n_terms; ++t) {
            const rmu_col_term& T = terms[t0 + t];
            d.field[t] = T.field; d.code_off[t] = off; d.n_codes[t] = T.codes_end - T.codes_begin;
            if (d.n_codes[t]) memcpy(hc + off, codes + T.codes_begin, (size_t)d.n_codes[t] * sizeof(int32_t));
            off += d.n_codes[t];
        }
        hs[i] = d;
    }
    RMU_HIP_TRY(hipMemcpyAsync(x.sels.p, x.pin.p, b_in, hipMemcpyHostToDevice, s));
    const ColSel* d_sels = (const ColSel*)x.sels.p;
    const int32_t* d_codes = (const int32_t*)((const char*)x.sels.p + b_sel);
    const bool timed = timing_on() && x.ensure_events();
    x.count_ms = x.write_ms = -1.f;
    x.wrote = false;
    if (timed) RMU_HIP_TRY(hipEventRecord(x.ev[0], s));
    hipLaunchKernelGGL(col_count_kernel, dim3((unsigned)n_tiles, (unsigned)n_named), dim3(kBlock), 0, s, (const int32_t*)c->img.p, c->cap_rows, n,
                       tile_rows, d_sels, d_codes, (u32*)x.counts.p, n_tiles);
    RMU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(col_scan_kernel<u32>, dim3((unsigned)n_named), dim3(kBlock), 0, s, (u32*)x.counts.p, (int64_t)n_tiles, (int64_t*)x.lptr.p);
    RMU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(col_scan_kernel<int64_t>, dim3(1), dim3(kBlock), 0, s, (int64_t*)x.lptr.p, (int64_t)n_named, (int64_t*)x.lptr.p + n_named);
    RMU_HIP_TRY(hipGetLastError());
    if (timed) RMU_HIP_TRY(hipEventRecord(x.ev[1], s));
    RMU_HIP_TRY(hipMemcpyAsync(x.pin.p, x.lptr.p, b_lp, hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    memcpy(lp, x.pin.p, b_lp);
    if (timed && hipEventElapsedTime(&x.count_ms, x.ev[0], x.ev[1]) != hipSuccess) x.count_ms = -1.f;
    return RMU_OK;
}

// pass 3 behind count_lists of the same call: the lists, end to end, into `out` (device, at least lp[n_named] entries); enqueues only
static int write_lists(rmu_columns* c, int64_t n, int n_named, int tile_rows, int n_tiles, int64_t* out, hipStream_t s) {
    Ctx& x = g_ctx;
    const size_t b_sel = (size_t)n_named * sizeof(ColSel);
    const bool timed = timing_on() && x.ensure_events();
    if (timed) RMU_HIP_TRY(hipEventRecord(x.ev[2], s));
    hipLaunchKernelGGL(col_write_kernel, dim3((unsigned)n_tiles, (unsigned)n_named), dim3(kBlock), 0, s, (const int32_t*)c->img.p, c->cap_rows, n,
                       tile_rows, (const ColSel*)x.sels.p, (const int32_t*)((const char*)x.sels.p + b_sel), (const u32*)x.counts.p, n_tiles,
                       (const int64_t*)x.lptr.p, out);
    RMU_HIP_TRY(hipGetLastError());
    if (timed) { RMU_HIP_TRY(hipEventRecord(x.ev[3], s)); x.wrote = true; }
    return RMU_OK;
}

// (internal, not in rmu.h; tools/where_probe.py) kernel times of the calling thread's last selection under RMU_COLUMNS_TIMING, once its
// stream is drained: passes 1 + 2, pass 3; < 0 = not taken
extern "C" int rmu_columns_last_ms_(float* count_ms, float* write_ms) {
    RMU_ENTRY();
    Ctx& x = g_ctx;
    if (x.write_ms < 0.f && x.wrote && hipEventElapsedTime(&x.write_ms, x.ev[2], x.ev[3]) != hipSuccess) {
        x.write_ms = -1.f;
        (void)hipGetLastError();
    }
    if (count_ms) *count_ms = x.count_ms;
    if (write_ms) *write_ms = x.write_ms;
    return RMU_OK;
}

// shared lock in, shared lock out: the image current for the rows the handle holds
static int settle_image(rmu_columns* c, std::shared_lock<std::shared_mutex>& lk, hipStream_t s) {
    while (c->n > 0 && (c->d_len != c->n || !c->img.p)) {
        lk.unlock();
        {
            std::unique_lock<std::shared_mutex> wl(c->mu);
            const int rc = upload_image(c, s);
            if (rc) { lk.lock(); return rc; }
        }
        lk.lock();
    }
    return RMU_OK;
}

// what a call that fails with work enqueued leaves behind: nothing in flight
static int drained(hipStream_t s, int rc) {
    (void)hipStreamSynchronize(s);
    rmu_thread_finished_(s, true);
    return rc;
}

extern "C" int rmu_columns_select(rmu_columns_t* c, const rmu_col_term* terms, int n_terms, const int32_t* codes, const int32_t* sel_ptr, int n_sel,
                                  unsigned flags, int64_t* out_rows, int64_t out_cap, int64_t* list_ptr, uint64_t hip_stream) {
    RMU_ENTRY();
    const std::string w("rmu_columns_select");
    if (!c) return rmu_fail(RMU_E_INVALID, w + ": null handle");
    if (!list_ptr) return rmu_fail(RMU_E_INVALID, w + ": list_ptr is null");
    if (flags & ~RMU_F_OUT_DEVICE) return rmu_fail(RMU_E_INVALID, w + ": the only flag is RMU_F_OUT_DEVICE");
    if (out_rows && out_cap < 0) return rmu_fail(RMU_E_INVALID, w + ": out_cap must be >= 0");
    int rc = check_selections(w, c->n_fields, terms, n_terms, codes, sel_ptr, n_sel);
    if (rc) return rc;
    hipStream_t s = nullptr;
    if ((rc = rmu_thread_stream_((hipStream_t)hip_stream, &s))) return rc;
    std::shared_lock<std::shared_mutex> lk(c->mu);
    if ((rc = settle_image(c, lk, s))) return drained(s, rc);
    const int64_t n = c->n;
    if (n == 0) {
        for (int g = 0; g <= n_sel; ++g) list_ptr[g] = 0;
        rmu_thread_finished_(s, true);
        return RMU_OK;
    }
    std::vector<int> named((size_t)n_sel);
    for (int g = 0; g < n_sel; ++g) named[g] = g;
    int tile_rows = 0, n_tiles = 0;
    if ((rc = count_lists(w, c, n, terms, codes, sel_ptr, named.data(), n_sel, s, list_ptr, &tile_rows, &n_tiles))) return drained(s, rc);
    const int64_t total = list_ptr[n_sel];
    if (!out_rows || total == 0) { rmu_thread_finished_(s, true); return RMU_OK; }
    if (out_cap < total) {
        rmu_thread_finished_(s, true);
        return rmu_fail(RMU_E_INVALID, w + ": out_cap (" + std::to_string(out_cap) + ") is smaller than the lists together (" + std::to_string(total) + " rows)");
    }
    int64_t* d_out = out_rows;
    if (!(flags & RMU_F_OUT_DEVICE)) {
        if (g_ctx.lists.ensure((size_t)total * sizeof(int64_t)) != hipSuccess) return drained(s, rmu_fail(RMU_E_OOM, w + ": list workspace"));
        d_out = (int64_t*)g_ctx.lists.p;
    }
    if ((rc = write_lists(c, n, n_sel, tile_rows, n_tiles, d_out, s))) return drained(s, rc);
    if (d_out != out_rows) {
        const hipError_t e = hipMemcpyAsync(out_rows, d_out, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return drained(s, rmu_fail(RMU_E_HIP, w + ": copy of the lists: " + hipGetErrorString(e)));
    }
    const hipError_t es = hipStreamSynchronize(s);
    rmu_thread_finished_(s, true);
    RMU_HIP_TRY(es);
    return RMU_OK;
}

extern "C" int rmu_index_search_where(rmu_index_t* idx, rmu_columns_t* c, const float* q, int64_t nq, int k, unsigned flags, int64_t row_base,
                                      const rmu_col_term* terms, int n_terms, const int32_t* codes, const int32_t* sel_ptr, int n_sel,
                                      const int32_t* q_sel, float* out_scores, int64_t* out_rows, uint64_t hip_stream) {
    RMU_ENTRY();
    const std::string w("rmu_index_search_where");
    if (!idx || !c || !q || !q_sel || !out_scores || !out_rows) return rmu_fail(RMU_E_INVALID, w + ": null pointer");
    if (nq < 1 || nq > kMaxSelections) return rmu_fail(RMU_E_INVALID, w + ": nq must be in [1, 8192]");
    if (k < 1 || k > RMU_MAX_K) return rmu_fail(RMU_E_INVALID, w + ": k must be in [1, 112]");
    if (flags & ~(RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE)) return rmu_fail(RMU_E_INVALID, w + ": the flags are RMU_F_Q_DEVICE and RMU_F_OUT_DEVICE");
    int rc = check_selections(w, c->n_fields, terms, n_terms, codes, sel_ptr, n_sel);
    if (rc) return rc;
    for (int64_t i = 0; i < nq; ++i)
        if (q_sel[i] < 0 || q_sel[i] >= n_sel || (i > 0 && q_sel[i] < q_sel[i - 1]))
            return rmu_fail(RMU_E_INVALID, w + ": q_sel must be non-decreasing selection numbers in [0, n_sel): entry " + std::to_string(i) +
                                           " names selection " + std::to_string(q_sel[i]));
    int dim = 0;
    if ((rc = rmu_index_dim(idx, &dim))) return rc;
    if (dim > RMU_MAX_DIM)
        return rmu_fail(RMU_E_INVALID, w + ": the index holds rows wider than 768 dimensions (RMU_MAX_DIM): the filtered search does not serve a wide index yet");
    // the selections some query names, and each query's list among them
    std::vector<int> named;
    std::vector<int32_t> q_list((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) {
        if (named.empty() || named.back() != q_sel[i]) named.push_back(q_sel[i]);
        q_list[i] = (int32_t)named.size() - 1;
    }
    const int n_named = (int)named.size();
    std::vector<int64_t> lp((size_t)n_named + 1, 0);

    hipStream_t s = nullptr;
    if ((rc = rmu_thread_stream_((hipStream_t)hip_stream, &s))) return rc;
    std::shared_lock<std::shared_mutex> lk(c->mu);
    int64_t idx_rows = 0;
    if ((rc = rmu_index_size(idx, &idx_rows))) return rc;
    if (idx_rows != c->n)
        return rmu_fail(RMU_E_INVALID, w + ": the columns (" + std::to_string(c->n) + " rows) and the index (" + std::to_string(idx_rows) + " rows) are out of step");
    if ((rc = settle_image(c, lk, s))) return drained(s, rc);
    const int64_t n = c->n;                    // (an append between the two locks: the lists name the rows both held at the check or later ones
                                               //  the index ignores -- a device list's ids outside [0, rows) are absent)
    const int64_t* d_lists = nullptr;
    if (n > 0) {
        int tile_rows = 0, n_tiles = 0;
        if ((rc = count_lists(w, c, n, terms, codes, sel_ptr, named.data(), n_named, s, lp.data(), &tile_rows, &n_tiles))) return drained(s, rc);
        const int64_t total = lp[n_named];
        if (total > 0) {
            if (g_ctx.lists.ensure((size_t)total * sizeof(int64_t)) != hipSuccess) return drained(s, rmu_fail(RMU_E_OOM, w + ": list workspace"));
            d_lists = (const int64_t*)g_ctx.lists.p;
            if ((rc = write_lists(c, n, n_named, tile_rows, n_tiles, (int64_t*)g_ctx.lists.p, s))) return drained(s, rc);
        }
    }
    // the gathered scan as it is: device lists, one per named selection; it drains s (the columns' shared lock is held until then)
    rc = rmu_index_search_groups(idx, q, nq, k, (flags & (RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE)) | RMU_F_ROWS_DEVICE, row_base, d_lists, lp.data(), n_named,
                                 q_list.data(), out_scores, out_rows, hip_stream);
    if (rc) return drained(s, rc);
    return RMU_OK;
}

// Grouped search (include/rmu.h): the codes of `field` name each row's group.  Here: every limit that needs no device, the columns' shared
// lock (held until the scan has drained: it reads the image), the image brought up to date; the scan, the fold and the finishing are
// rmu_api.hip's (rmu_index_search_distinct_on_), under the index's shared lock -- the lock order above.
extern "C" int rmu_index_search_distinct(rmu_index_t* idx, rmu_columns_t* c, int field, const float* q, int64_t nq, int k, unsigned flags,
                                         int64_t row_base, float* out_scores, int64_t* out_rows, uint64_t hip_stream) {
    RMU_ENTRY();
    const std::string w("rmu_index_search_distinct");
    if (!idx || !c || !q || !out_scores || !out_rows) return rmu_fail(RMU_E_INVALID, w + ": null pointer (idx, c, q, out_scores, out_rows)");
    if (nq < 1) return rmu_fail(RMU_E_INVALID, w + ": nq must be >= 1");
    if (k < 1 || k > RMU_MAX_K_DISTINCT) return rmu_fail(RMU_E_INVALID, w + ": k must be in [1, 32]");
    if (flags & ~(RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE)) return rmu_fail(RMU_E_INVALID, w + ": the flags are RMU_F_Q_DEVICE and RMU_F_OUT_DEVICE");
    if (field < 0 || field >= c->n_fields)
        return rmu_fail(RMU_E_INVALID, w + ": field " + std::to_string(field) + " is outside [0, " + std::to_string(c->n_fields) + ")");
    int rc, dim = 0;
    if ((rc = rmu_index_dim(idx, &dim))) return rc;
    if (dim > RMU_MAX_DIM)
        return rmu_fail(RMU_E_INVALID, w + ": the index holds rows wider than 768 dimensions (RMU_MAX_DIM): the grouped search does not serve a wide index");
    hipStream_t s = nullptr;
    if ((rc = rmu_thread_stream_((hipStream_t)hip_stream, &s))) return rc;
    std::shared_lock<std::shared_mutex> lk(c->mu);
    int64_t idx_rows = 0;
    if ((rc = rmu_index_size(idx, &idx_rows))) return rc;
    if (idx_rows != c->n)
        return rmu_fail(RMU_E_INVALID, w + ": the columns (" + std::to_string(c->n) + " rows) and the index (" + std::to_string(idx_rows) + " rows) are out of step");
    if ((rc = settle_image(c, lk, s))) return drained(s, rc);
    if (idx_rows != c->n)          // (an append while the lock was given up for the upload)
        return drained(s, rmu_fail(RMU_E_INVALID, w + ": the columns (" + std::to_string(c->n) + " rows) and the index (" + std::to_string(idx_rows) + " rows) are out of step"));
    const int32_t* codes = c->n > 0 ? (const int32_t*)c->img.p + (int64_t)field * c->cap_rows : nullptr;
    rc = rmu_index_search_distinct_on_(idx, codes, c->n, q, nq, k, flags, row_base, out_scores, out_rows, (hipStream_t)hip_stream);
    if (rc) return drained(s, rc);
    return RMU_OK;
}
