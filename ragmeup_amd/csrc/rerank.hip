// rerank.hip -- the rerank step by key: passage tokens in HBM, (query, passage) pairs assembled on the device, stable top-n on the device
// (gfx950 only).
//
// Serves: ContextualCompressionRetriever(base_compressor=ScoredCrossEncoderReranker, base_retriever=ensemble).invoke (server/RAGHelper.py:476-490,
// RAGHelper_local.py:157-159) and the same compressor run once more with the answer as the query (server/provenance.py:100-108): score every
// (query, page_content) pair with the cross-encoder, Python's stable sorted(..., reverse=True), keep top_n (ScoredCrossEncoderReranker.py:42-45).
//
// Passage table (rmu_passages_t): the WordPiece ids of every distinct passage text, WITHOUT special tokens, cut to the first max_len - 3 (the most
// "longest_first" can keep of the second text).  Each entry also remembers its length before the cut: which side of a pair receives the odd token
// of an odd budget depends on which side was LONGER, also when both are longer than the budget.  The host side (token vector, offsets, lengths) is
// the master and works with no device; the device image follows lazily: its first d_entries entries are current, the next rerank call uploads the
// tail under the exclusive lock, re-allocating (old contents copied on the device) when it does not fit.  Every reader holds the shared lock until
// it has drained its stream, so under the exclusive lock nothing reads the image and the old allocation can be freed at once: no reader events.
//
// pair_assemble_kernel: one wave per row of the batch; lane t writes positions t, t + 64, ... of [CLS] q [SEP] p [SEP] [PAD]..., token types 0 / 1,
// as rmu_tok_encode writes them; (n1, n2) by rmu_longest_first (pair_truncate.h), per pair, from the two lengths.  A key of -1 and a row past the
// pairs give length 0.  Keys are validated on the host against the table before anything is enqueued; offsets at set time.
//
// rerank_select_kernel: one 256-thread workgroup per query, m <= 256 logits in LDS; a candidate's slot is the number of present candidates with a
// greater logit, or an equal one at a lower position: the order of Python's stable sorted(reverse=True).  +0.0 == -0.0; a NaN ranks behind every
// number, NaNs among themselves by position.  O(m^2) compares on broadcast LDS reads, no atomics: deterministic.
#include <cmath>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/rmu.h"
#include "rmu_common.h"
#include "rmu_host.h"
#include "pair_truncate.h"
#include "rmu_internal.h"      // rmu_rerank_*_: the prototypes bert.hip calls them by


struct rmu_passages {
    int cls = 0, sep = 0, pad = 0, max_len = 0, cap = 0;      // cap = max_len - 3 tokens kept per entry
    // host side (the master): entry i = tok[off[i] .. off[i + 1]), flen[i] = its length before the cut
    std::vector<int32_t> tok;
    std::vector<int64_t> off{0};
    std::vector<int32_t> flen;
    // device image, same layout; entries [0, d_entries) are current
    int32_t* d_tok = nullptr;
    int64_t* d_off = nullptr;
    int32_t* d_flen = nullptr;
    size_t d_tok_cap = 0, d_ent_cap = 0;                       // tokens / entries the allocations hold (d_off: d_ent_cap + 1)
    size_t d_entries = 0;
    std::shared_mutex mu;
    size_t entries() const { return flen.size(); }
};

namespace {

constexpr int kAsmBlock = 256, kAsmRows = kAsmBlock / 64;      // pair_assemble_kernel: four rows (waves) per workgroup
constexpr int kSelBlock = 256;                                 // rerank_select_kernel: RMU_RERANK_MAX_M candidates, one per thread

struct AsmLaunch {
    const int32_t* tok;        // the table's image
    const int64_t* off;
    const int32_t* flen;
    const int32_t* q_tok;      // [nq, q_w] heads of the queries
    const int32_t* q_len;      // [nq] lengths before any cut
    const int64_t* keys;       // [pairs]
    int32_t *ids, *types, *lens;   // [rows, max_len] x 2, [rows]
    int pairs, rows, m, q_w, max_len, cls, sep, pad;
};

__global__ __launch_bounds__(kAsmBlock) void pair_assemble_kernel(AsmLaunch a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * kAsmRows + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int64_t key = row < a.pairs ? a.keys[row] : -1;
    int32_t* ids = a.ids + (size_t)row * a.max_len;
    int32_t* types = a.types + (size_t)row * a.max_len;
    if (key < 0) {
        for (int p = lane; p < a.max_len; p += 64) { ids[p] = a.pad; types[p] = 0; }
        if (lane == 0) a.lens[row] = 0;
        return;
    }
    const int q = row / a.m;
    const int64_t p0 = a.off[key];
    int n1, n2;
    rmu_longest_first(a.q_len[q], a.flen[key], a.max_len - 3, &n1, &n2);
    const int32_t* qt = a.q_tok + (size_t)q * a.q_w;
    const int32_t* pt = a.tok + p0;
    const int sep1 = 1 + n1, sep2 = sep1 + 1 + n2;
    for (int p = lane; p < a.max_len; p += 64) {
        int id, ty;
        if (p == 0) { id = a.cls; ty = 0; }
        else if (p < sep1) { id = qt[p - 1]; ty = 0; }
        else if (p == sep1) { id = a.sep; ty = 0; }
        else if (p < sep2) { id = pt[p - sep1 - 1]; ty = 1; }
        else if (p == sep2) { id = a.sep; ty = 1; }
        else { id = a.pad; ty = 0; }
        ids[p] = id;
        types[p] = ty;
    }
    if (lane == 0) a.lens[row] = sep2 + 1;
}

// a before b in Python's stable descending order (NaN behind every number); equal: neither is before the other
__device__ __forceinline__ bool sel_before(float a, float b) { return (a == a && b != b) || a > b; }
__device__ __forceinline__ bool sel_equal(float a, float b) { return (a != a && b != b) || a == b; }

__global__ __launch_bounds__(kSelBlock) void rerank_select_kernel(const float* logits, const int64_t* keys, int m, int top_n, int32_t* out_pos,
                                                                  float* out_scores) {
    __shared__ float s_v[kSelBlock];
    __shared__ int s_here[kSelBlock];
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x;
    const bool here = t < m && keys[q * m + t] >= 0;
    const float v = t < m ? logits[q * m + t] : 0.f;
    s_v[t] = v;
    s_here[t] = here ? 1 : 0;
    __syncthreads();
    int present = 0, slot = 0;
    for (int j = 0; j < m; ++j) {
        const bool hj = s_here[j] != 0;
        const float vj = s_v[j];
        present += hj ? 1 : 0;
        slot += (hj && (sel_before(vj, v) || (sel_equal(vj, v) && j < t))) ? 1 : 0;
    }
    const int64_t o = q * top_n;
    if (here && slot < top_n) {
        out_pos[o + slot] = t;
        out_scores[o + slot] = v;
    }
    for (int s = present + t; s < top_n; s += kSelBlock) {
        out_pos[o + s] = -1;
        out_scores[o + s] = -INFINITY;
    }
}

// per-thread workspaces.  Every call that uses them drains its stream before it returns (rmu_rerank_select with device inputs AND device outputs
// uses none), so nothing of a thread's previous call is ever in flight on them.
struct Ctx {
    RmuDevBuf in, work, out;      // queries | keys (| logits); assembled rows (+ logits) where the caller has no buffer of its own; positions | scores
    RmuPinBuf pin{8192};       // [0, pin_in): the inputs on their way up; behind it: the results on their way down
    int device = -1;
    // what the call in progress left for its later steps
    const int64_t* d_keys = nullptr;
    size_t pin_in = 0;
};
thread_local Ctx g_ctx;

size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }

// (shared lock held) everything a call asks of the table and of its own arrays, without touching HIP
int validate(const rmu_passages* p, const int32_t* q_lens, int64_t nq, int q_stride, const int64_t* keys, int m, int max_len, const std::string& w) {
    if (max_len < 8 || max_len > p->max_len) return rmu_fail(RMU_E_INVALID, w + ": 8 <= max_len <= the table's max_len (" + std::to_string(p->max_len) + ")");
    const int budget = max_len - 3;
    for (int64_t i = 0; i < nq; ++i) {
        if (q_lens[i] < 0) return rmu_fail(RMU_E_INVALID, w + ": a query length is negative");
        if ((q_lens[i] < budget ? q_lens[i] : budget) > q_stride)
            return rmu_fail(RMU_E_INVALID, w + ": q_stride is shorter than the head (max_len - 3 tokens) of a query");
    }
    const int64_t size = (int64_t)p->entries();
    for (int64_t i = 0; i < nq * m; ++i)
        if (keys[i] < -1 || keys[i] >= size)
            return rmu_fail(RMU_E_INVALID, w + ": key " + std::to_string(keys[i]) + " is outside the table (" + std::to_string(size) + " entries; -1 = absent)");
    return RMU_OK;
}

// (exclusive lock held: no reader of the image is in flight) bring the device image up to the host side; drains s
int upload_table(rmu_passages* p, hipStream_t s) {
    const size_t n = p->entries(), ntok = p->tok.size(), have = p->d_entries;
    const size_t have_tok = have ? (size_t)p->off[have] : 0;
    void* old[3] = {nullptr, nullptr, nullptr};
    if (ntok > p->d_tok_cap) {
        const size_t cap = ntok + ntok / 4 + 4096;
        int32_t* nt = nullptr;
        RMU_HIP_TRY(hipMalloc((void**)&nt, cap * sizeof(int32_t)));
        if (have_tok) (void)hipMemcpyAsync(nt, p->d_tok, have_tok * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
        old[0] = p->d_tok;
        p->d_tok = nt; p->d_tok_cap = cap;
    }
    if (n > p->d_ent_cap) {
        const size_t cap = n + n / 4 + 1024;
        int64_t* no = nullptr;
        int32_t* nf = nullptr;
        if (hipMalloc((void**)&no, (cap + 1) * sizeof(int64_t)) != hipSuccess || hipMalloc((void**)&nf, cap * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            if (no) (void)rmu_free(no);
            (void)hipStreamSynchronize(s);
            if (old[0]) (void)rmu_free(old[0]);                 // (its contents are in the new token array)
            return rmu_fail(RMU_E_OOM, "rmu_passages: device image of the offsets");
        }
        if (have) {
            (void)hipMemcpyAsync(no, p->d_off, (have + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(nf, p->d_flen, have * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
        }
        old[1] = p->d_off; old[2] = p->d_flen;
        p->d_off = no; p->d_flen = nf; p->d_ent_cap = cap;
    }
    if (n > have) {
        if (ntok > have_tok)
            (void)hipMemcpyAsync(p->d_tok + have_tok, p->tok.data() + have_tok, (ntok - have_tok) * sizeof(int32_t), hipMemcpyHostToDevice, s);
        (void)hipMemcpyAsync(p->d_off + have, p->off.data() + have, (n - have + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s);
        (void)hipMemcpyAsync(p->d_flen + have, p->flen.data() + have, (n - have) * sizeof(int32_t), hipMemcpyHostToDevice, s);
    }
    const hipError_t es = hipStreamSynchronize(s);             // (the host vectors are pageable; the old allocations have been copied from)
    for (void* o : old)
        if (o) (void)rmu_free(o);
    const hipError_t el = hipGetLastError();
    if (es != hipSuccess || el != hipSuccess) {
        p->d_entries = 0;                                       // whatever arrived: the next call uploads everything again
        return rmu_fail(RMU_E_HIP, std::string("rmu_passages: uploading the table: ") + hipGetErrorString(es != hipSuccess ? es : el));
    }
    p->d_entries = n;
    return RMU_OK;
}

// (shared lock held on entry and on return; validated) the image current, the queries and keys on the device, the assembly kernel enqueued on s.
// d_ids / d_types / d_lens: [rows, max_len] x 2, [rows] device; rows >= nq * m (the rows past the pairs get length 0); out_bytes: what the call
// will bring down through the pinned buffer behind the inputs (the buffer must not move once a copy out of it is in flight)
int assemble_enqueue(rmu_passages* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride, const int64_t* keys, int m, int rows,
                     int max_len, int32_t* d_ids, int32_t* d_types, int32_t* d_lens, size_t out_bytes, hipStream_t s,
                     std::shared_lock<std::shared_mutex>& lk, const std::string& w) {
    Ctx& x = g_ctx;
    int rc;
    while (p->d_entries != p->entries()) {
        lk.unlock();
        {
            std::unique_lock<std::shared_mutex> wl(p->mu);
            if ((rc = upload_table(p, s))) { wl.unlock(); lk.lock(); return rc; }
        }
        lk.lock();
        if ((rc = validate(p, q_lens, nq, q_stride, keys, m, max_len, w))) return rc;     // (a set may have run in between)
    }
    const int budget = max_len - 3;
    const int q_w = q_stride < budget ? q_stride : budget;
    const size_t pairs = (size_t)nq * m;
    const size_t b_tok = align8((size_t)nq * q_w * 4), b_len = align8((size_t)nq * 4), b_keys = pairs * 8;
    x.pin_in = b_tok + b_len + b_keys;
    if (x.pin.ensure(x.pin_in + out_bytes) != RMU_OK) return rmu_fail(RMU_E_OOM, w + ": pinned staging buffer");
    RMU_HIP_TRY(x.in.ensure(x.pin_in));
    for (int64_t i = 0; i < nq; ++i) memcpy(x.pin.p + (size_t)i * q_w * 4, q_tokens + (size_t)i * q_stride, (size_t)q_w * 4);
    memcpy(x.pin.p + b_tok, q_lens, (size_t)nq * 4);
    memcpy(x.pin.p + b_tok + b_len, keys, b_keys);
    RMU_HIP_TRY(hipMemcpyAsync(x.in.p, x.pin.p, x.pin_in, hipMemcpyHostToDevice, s));
    AsmLaunch a{};
    a.tok = p->d_tok; a.off = p->d_off; a.flen = p->d_flen;
    a.q_tok = (const int32_t*)x.in.p;
    a.q_len = (const int32_t*)((const char*)x.in.p + b_tok);
    a.keys = x.d_keys = (const int64_t*)((const char*)x.in.p + b_tok + b_len);
    a.ids = d_ids; a.types = d_types; a.lens = d_lens;
    a.pairs = (int)pairs; a.rows = rows; a.m = m; a.q_w = q_w; a.max_len = max_len;
    a.cls = p->cls; a.sep = p->sep; a.pad = p->pad;
    hipLaunchKernelGGL(pair_assemble_kernel, dim3((unsigned)((rows + kAsmRows - 1) / kAsmRows)), dim3(kAsmBlock), 0, s, a);
    RMU_HIP_TRY(hipGetLastError());
    return RMU_OK;
}

int check_call(const rmu_passages* p, const void* q_tokens, const void* q_lens, int64_t nq, int q_stride, const void* keys, int m, const std::string& w) {
    if (!p || !q_tokens || !q_lens || !keys) return rmu_fail(RMU_E_INVALID, w + ": null pointer");
    if (m < 1 || m > RMU_RERANK_MAX_M) return rmu_fail(RMU_E_INVALID, w + ": 1 <= m <= RMU_RERANK_MAX_M (256) candidates per query");
    if (nq < 1 || nq * m > 65535) return rmu_fail(RMU_E_INVALID, w + ": 1 <= nq, nq * m <= 65535 pairs");
    if (q_stride < 1) return rmu_fail(RMU_E_INVALID, w + ": q_stride must be >= 1");
    return RMU_OK;
}

}  // namespace

// ---- the table ----------------------------------------------------------------------------------------------------------------------------------
extern "C" int rmu_passages_create(rmu_passages_t** out, int cls_id, int sep_id, int pad_id, int max_len) {
    RMU_ENTRY();
    if (!out) return rmu_fail(RMU_E_INVALID, "rmu_passages_create: out is null");
    if (max_len < 8 || max_len > 512) return rmu_fail(RMU_E_INVALID, "rmu_passages_create: 8 <= max_len <= 512");
    if (cls_id < 0 || sep_id < 0 || pad_id < 0) return rmu_fail(RMU_E_INVALID, "rmu_passages_create: a special token id is negative");
    rmu_passages* p = new (std::nothrow) rmu_passages();
    if (!p) return rmu_fail(RMU_E_OOM, "rmu_passages_create: out of memory");
    p->cls = cls_id; p->sep = sep_id; p->pad = pad_id; p->max_len = max_len; p->cap = max_len - 3;
    *out = p;
    return RMU_OK;
}

extern "C" int rmu_passages_free(rmu_passages_t* p) {
    RMU_ENTRY();
    if (!p) return RMU_OK;
    {
        std::unique_lock<std::shared_mutex> lk(p->mu);          // readers end under the shared lock with their stream drained
        for (void* d : {(void*)p->d_tok, (void*)p->d_off, (void*)p->d_flen})
            if (d) (void)rmu_free(d);
    }
    delete p;
    return RMU_OK;
}

extern "C" int rmu_passages_size(rmu_passages_t* p, int64_t* n_entries, int64_t* n_tokens) {
    RMU_ENTRY();
    if (!p) return rmu_fail(RMU_E_INVALID, "rmu_passages_size: null handle");
    std::shared_lock<std::shared_mutex> lk(p->mu);
    if (n_entries) *n_entries = (int64_t)p->entries();
    if (n_tokens) *n_tokens = (int64_t)p->tok.size();
    return RMU_OK;
}

extern "C" int rmu_passages_set(rmu_passages_t* p, int64_t first, const int32_t* tokens, const int64_t* offsets, int64_t n) {
    RMU_ENTRY();
    if (!p || n < 0 || (n > 0 && !offsets)) return rmu_fail(RMU_E_INVALID, "rmu_passages_set: bad argument");
    std::unique_lock<std::shared_mutex> lk(p->mu);
    if (first < 0 || (uint64_t)first > p->entries())
        return rmu_fail(RMU_E_INVALID, "rmu_passages_set: first (" + std::to_string(first) + ") is beyond the table's length (" + std::to_string(p->entries()) +
                                        "): out of step");
    if (n > 0 && offsets[0] != 0) return rmu_fail(RMU_E_INVALID, "rmu_passages_set: offsets must start at 0");
    int64_t kept = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 0) return rmu_fail(RMU_E_INVALID, "rmu_passages_set: offsets must ascend");
        if (len > 0x7FFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_passages_set: an entry is longer than 2^31 - 1 tokens");
        kept += len < p->cap ? len : p->cap;
    }
    if (n > 0 && offsets[n] > 0 && !tokens) return rmu_fail(RMU_E_INVALID, "rmu_passages_set: tokens is null");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i], keep = len < p->cap ? len : p->cap;
        for (int64_t j = 0; j < keep; ++j)
            if (tokens[offsets[i] + j] < 0) return rmu_fail(RMU_E_INVALID, "rmu_passages_set: a token id is negative");
    }
    const size_t tok0 = (size_t)p->off[first];
    try {
        p->tok.reserve(tok0 + (size_t)kept);
        p->off.reserve((size_t)(first + n) + 1);
        p->flen.reserve((size_t)(first + n));
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_passages_set: out of memory"); }
    p->tok.resize(tok0);
    p->off.resize((size_t)first + 1);
    p->flen.resize((size_t)first);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i], keep = len < p->cap ? len : p->cap;
        if (keep) p->tok.insert(p->tok.end(), tokens + offsets[i], tokens + offsets[i] + keep);
        p->off.push_back((int64_t)p->tok.size());
        p->flen.push_back((int32_t)len);
    }
    if (p->d_entries > (size_t)first) p->d_entries = (size_t)first;
    return RMU_OK;
}

// ---- the assembled pairs themselves ---------------------------------------------------------------------------------------------------------------
extern "C" int rmu_passages_pairs(rmu_passages_t* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride, const int64_t* keys,
                                  int m, int max_len, int32_t* ids, int32_t* type_ids, int32_t* lens) {
    RMU_ENTRY();
    const std::string w = "rmu_passages_pairs";
    int rc = check_call(p, q_tokens, q_lens, nq, q_stride, keys, m, w);
    if (rc) return rc;
    if (!ids || !type_ids || !lens) return rmu_fail(RMU_E_INVALID, w + ": null pointer");
    std::shared_lock<std::shared_mutex> lk(p->mu);
    if ((rc = validate(p, q_lens, nq, q_stride, keys, m, max_len, w))) return rc;
    Ctx& x = g_ctx;
    rmu_follow_device(x.device);
    hipStream_t s = nullptr;
    if ((rc = rmu_thread_stream_(nullptr, &s))) return rc;
    const int rows = (int)(nq * m);
    const size_t cap = (size_t)rows * max_len;
    RMU_HIP_TRY(x.work.ensure((2 * cap + rows) * 4));
    int32_t* d_ids = (int32_t*)x.work.p;
    rc = assemble_enqueue(p, q_tokens, q_lens, nq, q_stride, keys, m, rows, max_len, d_ids, d_ids + cap, d_ids + 2 * cap, 0, s, lk, w);
    if (!rc) {
        (void)hipMemcpyAsync(ids, d_ids, cap * 4, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(type_ids, d_ids + cap, cap * 4, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(lens, d_ids + 2 * cap, (size_t)rows * 4, hipMemcpyDeviceToHost, s);
    }
    const hipError_t es = hipStreamSynchronize(s);
    rmu_thread_finished_(s, true);
    if (rc) return rc;
    RMU_HIP_TRY(es);
    RMU_HIP_TRY(hipGetLastError());
    return RMU_OK;
}

// ---- the selection ----------------------------------------------------------------------------------------------------------------------------------
extern "C" int rmu_rerank_select(const float* logits, const int64_t* keys, int64_t nq, int m, int top_n, unsigned flags, int32_t* out_pos,
                                 float* out_scores, uint64_t hip_stream) {
    RMU_ENTRY();
    if (!logits || !keys || !out_pos || !out_scores) return rmu_fail(RMU_E_INVALID, "rmu_rerank_select: null pointer");
    if (m < 1 || m > RMU_RERANK_MAX_M) return rmu_fail(RMU_E_INVALID, "rmu_rerank_select: 1 <= m <= RMU_RERANK_MAX_M (256) candidates per query");
    if (top_n < 1 || top_n > 65535) return rmu_fail(RMU_E_INVALID, "rmu_rerank_select: 1 <= top_n <= 65535");
    if (nq < 1 || nq > 65535) return rmu_fail(RMU_E_INVALID, "rmu_rerank_select: 1 <= nq <= 65535");
    if (flags & ~(unsigned)(RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE)) return rmu_fail(RMU_E_INVALID, "rmu_rerank_select: flags must be RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE");
    const bool in_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE;
    Ctx& x = g_ctx;
    rmu_follow_device(x.device);
    hipStream_t s = nullptr;
    int rc = rmu_thread_stream_((hipStream_t)hip_stream, &s);
    if (rc) return rc;
    const size_t nm = (size_t)nq * m, nk = (size_t)nq * top_n;
    const size_t b_keys = nm * 8, b_in = b_keys + nm * 4, b_out = nk * 8;
    if (x.pin.ensure((in_dev ? 0 : b_in) + (out_dev ? 0 : b_out)) != RMU_OK) return rmu_fail(RMU_E_OOM, "rmu_rerank_select: pinned staging buffer");
    const size_t pin_out = in_dev ? 0 : b_in;
    const float* d_logits = logits;
    const int64_t* d_keys = keys;
    if (!in_dev) {
        RMU_HIP_TRY(x.in.ensure(b_in));
        memcpy(x.pin.p, keys, b_keys);
        memcpy(x.pin.p + b_keys, logits, nm * 4);
        RMU_HIP_TRY(hipMemcpyAsync(x.in.p, x.pin.p, b_in, hipMemcpyHostToDevice, s));
        d_keys = (const int64_t*)x.in.p;
        d_logits = (const float*)((const char*)x.in.p + b_keys);
    }
    int32_t* d_pos = out_pos;
    float* d_scores = out_scores;
    if (!out_dev) {
        RMU_HIP_TRY(x.out.ensure(b_out));
        d_pos = (int32_t*)x.out.p;
        d_scores = (float*)(d_pos + nk);
    }
    hipLaunchKernelGGL(rerank_select_kernel, dim3((unsigned)nq), dim3(kSelBlock), 0, s, d_logits, d_keys, m, top_n, d_pos, d_scores);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !out_dev) e = hipMemcpyAsync(x.pin.p + pin_out, x.out.p, b_out, hipMemcpyDeviceToHost, s);
    const bool drained = e != hipSuccess || !hip_stream || !out_dev || !in_dev;
    if (drained) {
        const hipError_t es = hipStreamSynchronize(s);
        if (e == hipSuccess) e = es;
    }
    rmu_thread_finished_(s, drained);
    RMU_HIP_TRY(e);
    if (!out_dev) {
        memcpy(out_pos, x.pin.p + pin_out, nk * 4);
        memcpy(out_scores, x.pin.p + pin_out + nk * 4, nk * 4);
    }
    return RMU_OK;
}

// ---- bert.hip (rmu_bert_rerank): the same steps on the encoder's stream, in front of and behind its forward ------------------------------------
// every limit of the call but the model's, the table's under its shared lock -- which, with `lock` given, is handed back HELD (the caller
// releases it once it has drained the stream); no HIP call
extern "C" int rmu_rerank_check_(rmu_passages_t* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride, const int64_t* keys,
                                 int m, int batch_pad, int max_len, int top_n, const void* out_pos, const void* out_scores, void* lock) {
    const std::string w = "rmu_bert_rerank";
    if (m < 1 || m > RMU_RERANK_MAX_M) return rmu_fail(RMU_E_INVALID, w + ": 1 <= m_cand <= RMU_RERANK_MAX_M (256) candidates per query");
    if (top_n < 1 || top_n > 65535) return rmu_fail(RMU_E_INVALID, w + ": 1 <= top_n <= 65535");
    int rc = check_call(p, q_tokens, q_lens, nq, q_stride, keys, m, w);
    if (rc) return rc;
    if (!out_pos || !out_scores) return rmu_fail(RMU_E_INVALID, w + ": null pointer");
    if (batch_pad < nq * m || batch_pad > 65535) return rmu_fail(RMU_E_INVALID, w + ": nq * m_cand <= batch_pad <= 65535");
    std::shared_lock<std::shared_mutex> lk(p->mu);
    if ((rc = validate(p, q_lens, nq, q_stride, keys, m, max_len, w))) return rc;
    if (lock) *(std::shared_lock<std::shared_mutex>*)lock = std::move(lk);
    return RMU_OK;
}
// the thread's workspace for the shapes the encoder's own staging does not hold: ids | type ids | lens | logits of batch_pad rows
extern "C" int rmu_rerank_workspace_(int batch_pad, int max_len, int32_t** d_in, float** d_logits) {
    Ctx& x = g_ctx;
    rmu_follow_device(x.device);
    const size_t cap = (size_t)batch_pad * max_len;
    RMU_HIP_TRY(x.work.ensure((2 * cap + 2 * (size_t)batch_pad) * 4));
    *d_in = (int32_t*)x.work.p;
    *d_logits = (float*)(*d_in + 2 * cap + batch_pad);
    return RMU_OK;
}
// d_in: ids [batch_pad, max_len] | type ids | lens [batch_pad] (the encoder's staging layout)
extern "C" int rmu_rerank_assemble_(rmu_passages_t* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride, const int64_t* keys,
                                    int m, int batch_pad, int max_len, int top_n, int32_t* d_in, void* hip_stream, void* lock) {
    Ctx& x = g_ctx;
    rmu_follow_device(x.device);
    const size_t cap = (size_t)batch_pad * max_len, nm = (size_t)nq * m, nk = (size_t)nq * top_n;
    RMU_HIP_TRY(x.out.ensure(nk * 8));                               // (nothing of this call is in flight yet: a re-allocation disturbs nothing)
    return assemble_enqueue(p, q_tokens, q_lens, nq, q_stride, keys, m, batch_pad, max_len, d_in, d_in + cap, d_in + 2 * cap, nk * 8 + nm * 4,
                            (hipStream_t)hip_stream, *(std::shared_lock<std::shared_mutex>*)lock, "rmu_bert_rerank");
}
// behind the forward: the selection over d_logits [nq * m] and the keys the assembly left on the device; results (and the logits) on their way
// to pinned memory
extern "C" int rmu_rerank_select_(const float* d_logits, int64_t nq, int m, int top_n, int want_logits, void* hip_stream) {
    Ctx& x = g_ctx;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t nm = (size_t)nq * m, nk = (size_t)nq * top_n;
    if (x.pin_in + nk * 8 + nm * 4 > x.pin.cap || nk * 8 > x.out.cap) return rmu_fail(RMU_E_INVALID, "rmu_bert_rerank: the selection does not follow its assembly");
    int32_t* d_pos = (int32_t*)x.out.p;
    hipLaunchKernelGGL(rerank_select_kernel, dim3((unsigned)nq), dim3(kSelBlock), 0, s, d_logits, x.d_keys, m, top_n, d_pos, (float*)(d_pos + nk));
    RMU_HIP_TRY(hipGetLastError());
    RMU_HIP_TRY(hipMemcpyAsync(x.pin.p + x.pin_in, x.out.p, nk * 8, hipMemcpyDeviceToHost, s));
    if (want_logits) RMU_HIP_TRY(hipMemcpyAsync(x.pin.p + x.pin_in + nk * 8, d_logits, nm * 4, hipMemcpyDeviceToHost, s));
    return RMU_OK;
}
// (the stream is drained)
extern "C" void rmu_rerank_take_(int64_t nq, int m, int top_n, int32_t* out_pos, float* out_scores, float* out_logits) {
    const Ctx& x = g_ctx;
    const size_t nm = (size_t)nq * m, nk = (size_t)nq * top_n;
    const char* src = x.pin.p + x.pin_in;
    memcpy(out_pos, src, nk * 4);
    memcpy(out_scores, src + nk * 4, nk * 4);
    if (out_logits) memcpy(out_logits, src + nk * 8, nm * 4);
}
