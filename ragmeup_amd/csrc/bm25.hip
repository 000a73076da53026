// bm25.hip -- Okapi BM25 over an inverted index that lives in HBM: host-side index building + one fused "score postings, select top-k"
// kernel (gfx950 only).
//
// Serves the sparse half of the reference's retrieval ensemble: BM25Retriever.from_texts(...) inside
// EnsembleRetriever([sparse, dense], weights=[0.5, 0.5]) (server/RAGHelper.py:436-443, :492-505, rebuilt from scratch after every upload at
// :529-531).  Restates rank_bm25.BM25Okapi as langchain's BM25Retriever drives it, from the published formula:
//   tokens   = Python's str.split(): maximal runs of non-whitespace, whitespace = what str.isspace() accepts (U+0009-000D, 001C-001F, 0020,
//              0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000); case-sensitive, nothing stripped; an empty document has length 0
//   idf[t]   = ln(N - df + 0.5) - ln(df + 0.5) in double; every idf < 0 is replaced by epsilon * mean(idf over the vocabulary, before replacement)
//   score    = sum over the query's tokens IN ORDER, duplicates counted each time, unknown tokens contributing 0, of
//              idf[t] * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl))
//   result   = every document is a candidate (zero and negative scores included); slots beyond N hold (-inf, -1) as in rmu_index_search.
// ORDER OF TIES: the project's own -- score descending, then LOWER document id.  rank_bm25's get_top_n (argsort()[::-1]) puts the HIGHER id
// first among equal scores and is not stable; documents with equal scores may therefore come back in another order than the reference's.
// Out of scope: deleting documents, persistence (the reference pickles its chunks and rebuilds the retriever), the ParadeDB SQL retriever.
//
// Host (plain C++, no HIP: testable without a GPU): whitespace tokenizer over a NUL-separated blob, term -> id map, per-term master posting
// vectors (ascending document id, tf) and dl.  Adding documents appends; document ids are insertion order.
// Device image, built lazily by the first search after an add (one packed copy per dirty search; the reference rebuilds its whole retriever per
// upload): post_doc[nnz] u32, post_tf[nnz] u32, doc_norm[N] fp32 = k1 * (1 - b + b * dl / avgdl) computed in double.  post_ptr[V + 1] and the
// fp32 term weights idf * (k1 + 1) stay on the host: a search resolves its terms there and ships (posting begin, length, weight) descriptors.
// The image is swapped under the handle's exclusive lock.  Every search hands HOST results back, i.e. it drains its stream before it returns and
// does so under the shared lock: a writer that holds the exclusive lock has no reader left in flight to wait for.
//
// Kernel (bm25_topk_kernel): grid = (workgroups over the document axis, queries).  A workgroup owns a contiguous range of documents and walks it
// in tiles of `tile` documents whose fp32 accumulators sit in LDS.  Per tile it loops over the query's terms in query order with a barrier
// between terms: inside one term a document occurs once, so lanes update distinct LDS words with a plain read-modify-write -- no atomics, and
// a document's score is ((0 + c_1) + c_2) + ... over the terms that hold it, whatever the tile size, the grid or the batch.  One cursor per
// term lives in LDS; it is found by ONE binary search per (workgroup, term) and then only advances.  doc_norm is gathered per posting (a tile
// without postings reads none of it).  Selection: each wave folds its 64-document batches into a running sorted top list (rmu_common.h's
// bitonic helpers) and skips, with one ballot, every batch in which no key beats its current k-th; the waves combine through LDS at the end of
// the range; the workgroup writes one sorted, zero-padded list [part, q, k], and rmu_merge_final_launch (topk_merge.hip) finishes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rmu.h"
#include "rmu_common.h"

extern "C" void rmu_set_error_(const char* msg);
static int mfail(int code, const std::string& m) { rmu_set_error_(m.c_str()); return code; }
#define BM25_TRY(expr)                                                                                              \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess)                                                                                       \
            return mfail(e_ == hipErrorOutOfMemory ? RMU_E_OOM : RMU_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace {

constexpr int kMaxTile = 8192;      // documents per tile: 32 KiB of accumulators
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxTerms = 1024;     // tokens per query
constexpr int kMaxParts = 1024;     // workgroups per query = part lists of the final merge (tests/merge_regimes.py pins it up to 1040)

struct TermDesc {
    u64 begin;   // first posting of the term in post_doc / post_tf
    u32 len;     // its postings (= df)
    float w;     // fp32(idf * (k1 + 1))
};
static_assert(sizeof(TermDesc) == 16, "descriptor layout");

struct Bm25Launch {
    const u32* post_doc;
    const u32* post_tf;
    const float* doc_norm;
    const u32* term_ptr;     // [nq + 1]: query q's descriptors are terms[term_ptr[q] .. term_ptr[q + 1])
    const TermDesc* terms;
    u64* partial;            // [parts, nq, k]
    u32 n_docs;
    int nq, k, tile, tiles_per_wg;
};

// fold one 64-key batch into the running sorted list (the step of topk_merge.hip's merge_stream)
template <int NPL>
__device__ __forceinline__ void fold64(u64 (&top)[NPL], u64 key, int lane) {
    u64 bk[1] = {key};
    rmu_bitonic_sort_desc<1>(bk, lane);
    const u64 rev = __shfl(bk[0], 63 - lane);
    u64& tail = top[NPL - 1];
    tail = tail > rev ? tail : rev;
    rmu_bitonic_merge_desc<NPL>(top, lane);
}
template <int NPL>
__device__ __forceinline__ u64 kth_of(const u64 (&top)[NPL], int k) {
    const u64 v = (NPL > 1 && k > 64) ? top[NPL - 1] : top[0];
    return __shfl(v, (k - 1) & 63);
}

template <int NPL>
__global__ __launch_bounds__(kBlock) void bm25_topk_kernel(Bm25Launch p) {
    __shared__ __attribute__((aligned(16))) float acc[kMaxTile];
    __shared__ u32 cur[kMaxTerms];
    __shared__ u32 wcnt[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = blockIdx.y;
    const u32 tb = p.term_ptr[q];
    const int nt = (int)(p.term_ptr[q + 1] - tb);
    const TermDesc* __restrict__ terms = p.terms + tb;
    const int64_t d_lo = (int64_t)blockIdx.x * p.tiles_per_wg * p.tile;
    const int64_t d_end = d_lo + (int64_t)p.tiles_per_wg * p.tile;
    const int64_t d_hi = d_end < (int64_t)p.n_docs ? d_end : (int64_t)p.n_docs;

    // the only search: first posting >= d_lo of every term, one lane per term
    for (int t = tid; t < nt; t += kBlock) {
        const TermDesc td = terms[t];
        const u32* __restrict__ pd = p.post_doc + td.begin;
        u32 lo = 0, hi = td.len;
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if ((int64_t)pd[mid] < d_lo) lo = mid + 1;
            else hi = mid;
        }
        cur[t] = lo;
    }

    u64 top[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) top[i] = 0ull;
    u64 kth = 0ull;

    for (int64_t t0 = d_lo; t0 < d_hi; t0 += p.tile) {
        const int64_t t1 = t0 + p.tile < d_hi ? t0 + p.tile : d_hi;
        const int cnt = (int)(t1 - t0);
        __syncthreads();                       // the selection of the tile before has read acc
        for (int j = tid; j < cnt; j += kBlock) acc[j] = 0.f;
        __syncthreads();
        u32 prev_c = 0;
        for (int t = 0; t < nt; ++t) {
            const TermDesc td = terms[t];
            const u32 c = cur[t];
            // the term before is complete (barrier below): its cursor moves past what the waves consumed
            if (t > 0 && tid == 0) cur[t - 1] = prev_c + wcnt[(t - 1) & 1][0] + wcnt[(t - 1) & 1][1] + wcnt[(t - 1) & 1][2] + wcnt[(t - 1) & 1][3];
            const u32* __restrict__ pd = p.post_doc + td.begin;
            const u32* __restrict__ pf = p.post_tf + td.begin;
            u32 total = 0;
            // wave w streams the 64-posting chunks w, w + 4, ... from the cursor; postings ascend, so the chunks inside the tile are a prefix
            for (u32 i = c + (u32)(w * 64 + lane);; i += kBlock) {
                bool in = false;
                u32 doc = 0;
                if (i < td.len) {
                    doc = pd[i];
                    in = (int64_t)doc < t1;
                }
                if (in) {
                    const u32 off = doc - (u32)t0;
                    if (off < (u32)cnt) {
                        const float tf = (float)pf[i];
                        acc[off] += (td.w * tf) / (tf + p.doc_norm[doc]);
                    }
                }
                const u64 b = __ballot(in);
                total += (u32)__builtin_popcountll(b);
                if (b != ~0ull) break;
            }
            if (lane == 0) wcnt[t & 1][w] = total;
            prev_c = c;
            __syncthreads();
        }
        if (nt > 0 && tid == 0) cur[nt - 1] = prev_c + wcnt[(nt - 1) & 1][0] + wcnt[(nt - 1) & 1][1] + wcnt[(nt - 1) & 1][2] + wcnt[(nt - 1) & 1][3];
        // selection: wave w takes the 64-document batches w, w + 4, ... of the tile
        for (int j0 = w * 64; j0 < cnt; j0 += kBlock) {
            const int j = j0 + lane;
            const u64 key = j < cnt ? rmu_make_key(acc[j], (u32)(t0 + j)) : 0ull;
            if (!__any(key > kth)) continue;
            fold64<NPL>(top, key, lane);
            kth = kth_of<NPL>(top, p.k);
        }
    }

    // the waves' lists -> one list of the workgroup
    __syncthreads();
    u64* lists = reinterpret_cast<u64*>(acc);
#pragma unroll
    for (int i = 0; i < NPL; ++i) lists[(w * NPL + i) * 64 + lane] = top[i];
    __syncthreads();
    if (w != 0) return;
    for (int b = NPL; b < kWaves * NPL; ++b) {
        const u64 key = lists[b * 64 + lane];
        if (!__any(key > kth)) continue;
        fold64<NPL>(top, key, lane);
        kth = kth_of<NPL>(top, p.k);
    }
    u64* out = p.partial + ((int64_t)blockIdx.x * p.nq + q) * p.k;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int e = lane + 64 * i;
        if (e < p.k) out[e] = top[i];
    }
}

// ---- host: tokenizer and index ---------------------------------------------------------------------------------------------------------
// length in bytes of the str.isspace() character at p (n bytes left), 0 if there is none.  The multi-byte forms cannot occur inside another
// character of valid UTF-8, so matching bytes is matching code points.
inline int space_len(const unsigned char* p, size_t n) {
    const unsigned c = p[0];
    if (c < 0x80) return ((c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20)) ? 1 : 0;
    if (c == 0xC2) return (n >= 2 && (p[1] == 0x85 || p[1] == 0xA0)) ? 2 : 0;
    if (n < 3) return 0;
    if (c == 0xE1) return (p[1] == 0x9A && p[2] == 0x80) ? 3 : 0;                                   // U+1680
    if (c == 0xE2) {
        if (p[1] == 0x80) return ((p[2] >= 0x80 && p[2] <= 0x8A) || p[2] == 0xA8 || p[2] == 0xA9 || p[2] == 0xAF) ? 3 : 0;   // U+2000-200A, 2028, 2029, 202F
        return (p[1] == 0x81 && p[2] == 0x9F) ? 3 : 0;                                              // U+205F
    }
    if (c == 0xE3) return (p[1] == 0x80 && p[2] == 0x80) ? 3 : 0;                                   // U+3000
    return 0;
}
// fn(token bytes, length) for every token of s[0, n)
template <class Fn>
void split_tokens(const char* s, size_t n, Fn fn) {
    const unsigned char* p = (const unsigned char*)s;
    size_t i = 0, start = 0;
    bool open = false;
    while (i < n) {
        const int sl = space_len(p + i, n - i);
        if (sl) {
            if (open) { fn(s + start, i - start); open = false; }
            i += (size_t)sl;
        } else {
            if (!open) { start = i; open = true; }
            ++i;
        }
    }
    if (open) fn(s + start, n - start);
}
// the n NUL-terminated strings of a blob (rmu_tok_encode_blob's convention); false unless it holds exactly n of them
bool split_blob(const char* blob, int64_t bytes, int64_t n, std::vector<std::pair<const char*, size_t>>& out) {
    out.reserve((size_t)n);
    const char* p = blob;
    const char* e = blob + bytes;
    while (p < e && (int64_t)out.size() < n) {
        const char* z = (const char*)memchr(p, 0, (size_t)(e - p));
        if (!z) return false;
        out.emplace_back(p, (size_t)(z - p));
        p = z + 1;
    }
    return (int64_t)out.size() == n && p == e;
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)rmu_free(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        const hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
};
bool g_bm25_down = false;      // static destructors have begun: thread-local destructors must leave HIP alone
struct DownGuard { ~DownGuard() { g_bm25_down = true; } } g_down_guard;
// per-thread stream and workspaces of rmu_bm25_search (every call drains its stream, so nothing of a thread's is ever in flight between calls)
struct Ctx {
    hipStream_t stream = nullptr;
    int device = -1;
    DevBuf stage, partial, out;
    char* pin = nullptr;
    size_t pin_cap = 0;
    int ensure_stream() {
        const int dev = rmu_device_ordinal();
        if (dev >= 0 && device != dev) { (void)hipSetDevice(dev); device = dev; }
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { stream = nullptr; return RMU_E_HIP; }
        return RMU_OK;
    }
    int ensure_pin(size_t bytes) {
        if (bytes <= pin_cap) return RMU_OK;
        if (pin) (void)hipHostFree(pin);
        pin = nullptr; pin_cap = 0;
        const size_t cap = bytes < 4096 ? 4096 : bytes * 2;
        if (hipHostMalloc((void**)&pin, cap) != hipSuccess) { pin = nullptr; (void)hipGetLastError(); return RMU_E_OOM; }
        pin_cap = cap;
        return RMU_OK;
    }
    ~Ctx() {
        if (g_bm25_down) return;
        RMU_ENTRY();
        if (stream) (void)hipStreamSynchronize(stream);
        for (DevBuf* b : {&stage, &partial, &out})
            if (b->p) (void)rmu_free(b->p);
        if (pin) (void)hipHostFree(pin);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
thread_local Ctx g_ctx;

}  // namespace

struct rmu_bm25 {
    double k1 = 1.5, b = 0.75, epsilon = 0.25;
    std::unordered_map<std::string, u32> ids;      // term -> id, ids in order of first occurrence
    struct Postings { std::vector<u32> doc, tf; };
    std::vector<Postings> terms;                   // master posting vectors, ascending document id
    std::vector<u32> dl;
    uint64_t total_len = 0, nnz = 0;
    bool broken = false;                           // an allocation failed half-way through an add
    int64_t opt_tile = 0, opt_max_wgs = 0;
    // device image + the host half of it (valid while !dirty)
    bool dirty = true;
    u32* post_doc = nullptr;
    u32* post_tf = nullptr;
    float* doc_norm = nullptr;
    std::vector<u64> post_ptr;                     // [V + 1]
    std::vector<float> weight;                     // [V] fp32(idf * (k1 + 1))
    std::shared_mutex mu;
};

static void drop_image(rmu_bm25* h) {
    for (void* p : {(void*)h->post_doc, (void*)h->post_tf, (void*)h->doc_norm})
        if (p) (void)rmu_free(p);
    h->post_doc = h->post_tf = nullptr;
    h->doc_norm = nullptr;
    h->dirty = true;
}

// (exclusive lock held) pack the master vectors and upload them; no search is in flight (see the header)
static int build_image(rmu_bm25* h, hipStream_t s) {
    drop_image(h);
    const size_t V = h->terms.size(), N = h->dl.size();
    std::vector<u32> pk;          // post_doc | post_tf
    std::vector<float> norm;
    try {
        h->post_ptr.assign(V + 1, 0);
        h->weight.assign(V, 0.f);
        pk.resize(2 * (size_t)h->nnz);
        norm.resize(N);
    } catch (...) { return mfail(RMU_E_OOM, "rmu_bm25_search: out of memory while packing the index"); }
    u32* pdoc = pk.data();
    u32* ptf = pk.data() + h->nnz;
    std::vector<double> idf(V);
    double idf_sum = 0.0;
    u64 at = 0;
    for (size_t t = 0; t < V; ++t) {
        const auto& ps = h->terms[t];
        const double df = (double)ps.doc.size();
        idf[t] = std::log((double)N - df + 0.5) - std::log(df + 0.5);
        idf_sum += idf[t];
        h->post_ptr[t] = at;
        if (!ps.doc.empty()) {
            memcpy(pdoc + at, ps.doc.data(), ps.doc.size() * sizeof(u32));
            memcpy(ptf + at, ps.tf.data(), ps.tf.size() * sizeof(u32));
        }
        at += ps.doc.size();
    }
    h->post_ptr[V] = at;
    const double repl = V ? h->epsilon * (idf_sum / (double)V) : 0.0;
    for (size_t t = 0; t < V; ++t) h->weight[t] = (float)((idf[t] < 0.0 ? repl : idf[t]) * (h->k1 + 1.0));
    const double avgdl = N ? (double)h->total_len / (double)N : 0.0;
    for (size_t d = 0; d < N; ++d)
        norm[d] = (float)(h->k1 * (1.0 - h->b + (avgdl > 0.0 ? h->b * (double)h->dl[d] / avgdl : 0.0)));
    const size_t pbytes = (size_t)h->nnz * sizeof(u32);
    BM25_TRY(hipMalloc((void**)&h->post_doc, pbytes ? pbytes : 4));
    BM25_TRY(hipMalloc((void**)&h->post_tf, pbytes ? pbytes : 4));
    BM25_TRY(hipMalloc((void**)&h->doc_norm, N ? N * sizeof(float) : 4));
    if (pbytes) {
        BM25_TRY(hipMemcpyAsync(h->post_doc, pdoc, pbytes, hipMemcpyHostToDevice, s));
        BM25_TRY(hipMemcpyAsync(h->post_tf, ptf, pbytes, hipMemcpyHostToDevice, s));
    }
    if (N) BM25_TRY(hipMemcpyAsync(h->doc_norm, norm.data(), N * sizeof(float), hipMemcpyHostToDevice, s));
    BM25_TRY(hipStreamSynchronize(s));
    h->dirty = false;
    return RMU_OK;
}

extern "C" int rmu_bm25_create(rmu_bm25_t** out, double k1, double b, double epsilon) {
    RMU_ENTRY();
    if (!out) return mfail(RMU_E_INVALID, "rmu_bm25_create: null argument");
    if (!(k1 >= 0.0) || !std::isfinite(k1) || !(b >= 0.0 && b <= 1.0) || !std::isfinite(epsilon))
        return mfail(RMU_E_INVALID, "rmu_bm25_create: k1 must be finite and >= 0, b in [0, 1], epsilon finite");
    rmu_bm25* h = new (std::nothrow) rmu_bm25();
    if (!h) return mfail(RMU_E_OOM, "rmu_bm25_create: out of memory");
    h->k1 = k1; h->b = b; h->epsilon = epsilon;
    *out = h;
    return RMU_OK;
}

extern "C" int rmu_bm25_free(rmu_bm25_t* h) {
    RMU_ENTRY();
    if (!h) return RMU_OK;
    {
        std::unique_lock<std::shared_mutex> lk(h->mu);      // searches end under the shared lock with their streams drained
        drop_image(h);
    }
    delete h;
    return RMU_OK;
}

extern "C" int rmu_bm25_add_texts(rmu_bm25_t* h, const char* blob, int64_t bytes, int64_t n, int64_t* first_doc) {
    RMU_ENTRY();
    if (!h || n < 0 || bytes < n || (n > 0 && !blob)) return mfail(RMU_E_INVALID, "rmu_bm25_add_texts: bad argument");
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (h->broken) return mfail(RMU_E_OOM, "rmu_bm25_add_texts: an earlier add ran out of memory, the index is unusable");
    if ((uint64_t)h->dl.size() + (uint64_t)n > 0x7FFFFFFFull) return mfail(RMU_E_INVALID, "rmu_bm25_add_texts: more than 2^31 - 1 documents");
    if (first_doc) *first_doc = (int64_t)h->dl.size();
    if (n == 0) {
        if (bytes != 0) return mfail(RMU_E_INVALID, "rmu_bm25_add_texts: the blob does not hold exactly n NUL-terminated strings");
        return RMU_OK;
    }
    try {
        std::vector<std::pair<const char*, size_t>> docs;
        if (!split_blob(blob, bytes, n, docs)) return mfail(RMU_E_INVALID, "rmu_bm25_add_texts: the blob does not hold exactly n NUL-terminated strings");
        h->dirty = true;
        h->broken = true;                       // until the add is complete
        std::vector<u32> seen;
        std::string key;
        for (const auto& d : docs) {
            const u32 id = (u32)h->dl.size();
            seen.clear();
            split_tokens(d.first, d.second, [&](const char* p, size_t len) {
                key.assign(p, len);
                auto it = h->ids.find(key);
                if (it == h->ids.end()) {
                    it = h->ids.emplace(key, (u32)h->terms.size()).first;
                    h->terms.emplace_back();
                }
                seen.push_back(it->second);
            });
            std::sort(seen.begin(), seen.end());
            for (size_t i = 0; i < seen.size();) {
                size_t j = i;
                while (j < seen.size() && seen[j] == seen[i]) ++j;
                auto& ps = h->terms[seen[i]];
                ps.doc.push_back(id);
                ps.tf.push_back((u32)(j - i));
                ++h->nnz;
                i = j;
            }
            h->dl.push_back((u32)seen.size());
            h->total_len += seen.size();
        }
        h->broken = false;
    } catch (...) { return mfail(RMU_E_OOM, "rmu_bm25_add_texts: out of memory, the index is unusable"); }
    return RMU_OK;
}

extern "C" int rmu_bm25_stat(rmu_bm25_t* h, int what, double* out) {
    RMU_ENTRY();
    if (!h || !out) return mfail(RMU_E_INVALID, "rmu_bm25_stat: null argument");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    switch (what) {
        case RMU_BM25_STAT_DOCS: *out = (double)h->dl.size(); break;
        case RMU_BM25_STAT_VOCAB: *out = (double)h->terms.size(); break;
        case RMU_BM25_STAT_NNZ: *out = (double)h->nnz; break;
        case RMU_BM25_STAT_AVGDL: *out = h->dl.empty() ? 0.0 : (double)h->total_len / (double)h->dl.size(); break;
        default: return mfail(RMU_E_INVALID, "rmu_bm25_stat: unknown statistic");
    }
    return RMU_OK;
}

extern "C" int rmu_bm25_df(rmu_bm25_t* h, const char* term_utf8, int64_t* df) {
    RMU_ENTRY();
    if (!h || !term_utf8 || !df) return mfail(RMU_E_INVALID, "rmu_bm25_df: null argument");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    try {
        const auto it = h->ids.find(term_utf8);
        *df = it == h->ids.end() ? 0 : (int64_t)h->terms[it->second].doc.size();
    } catch (...) { return mfail(RMU_E_OOM, "rmu_bm25_df: out of memory"); }
    return RMU_OK;
}

extern "C" int rmu_bm25_set_option(rmu_bm25_t* h, int option, int64_t value) {
    RMU_ENTRY();
    if (!h) return mfail(RMU_E_INVALID, "rmu_bm25_set_option: null handle");
    std::unique_lock<std::shared_mutex> lk(h->mu);
    switch (option) {
        case RMU_BM25_OPT_TILE_DOCS:
            if (value != 0 && (value < 64 || value > kMaxTile || (value & (value - 1))))
                return mfail(RMU_E_INVALID, "rmu_bm25_set_option: RMU_BM25_OPT_TILE_DOCS takes 0 or a power of two in [64, 8192]");
            h->opt_tile = value;
            break;
        case RMU_BM25_OPT_MAX_WGS:
            if (value < 0 || value > kMaxParts) return mfail(RMU_E_INVALID, "rmu_bm25_set_option: RMU_BM25_OPT_MAX_WGS takes 0 .. 1024");
            h->opt_max_wgs = value;
            break;
        default: return mfail(RMU_E_INVALID, "rmu_bm25_set_option: unknown option");
    }
    return RMU_OK;
}

extern "C" int rmu_bm25_search(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, float* out_scores,
                               int64_t* out_docs, uint64_t hip_stream) {
    RMU_ENTRY();
    if (!h || !query_blob || !out_scores || !out_docs) return mfail(RMU_E_INVALID, "rmu_bm25_search: null argument");
    if (nq < 1 || nq > 65535 || bytes < nq) return mfail(RMU_E_INVALID, "rmu_bm25_search: 1 <= nq <= 65535 queries, each NUL-terminated");
    if (k < 1 || k > RMU_MAX_K) return mfail(RMU_E_INVALID, "rmu_bm25_search: 1 <= k <= RMU_MAX_K");
    std::vector<std::pair<const char*, size_t>> qs;
    std::vector<std::vector<std::string>> toks;
    try {
        if (!split_blob(query_blob, bytes, nq, qs)) return mfail(RMU_E_INVALID, "rmu_bm25_search: the blob does not hold exactly nq NUL-terminated strings");
        toks.resize((size_t)nq);
        for (int64_t i = 0; i < nq; ++i) {
            split_tokens(qs[i].first, qs[i].second, [&](const char* p, size_t len) { toks[i].emplace_back(p, len); });
            if (toks[i].size() > (size_t)kMaxTerms) return mfail(RMU_E_INVALID, "rmu_bm25_search: a query has more than 1024 tokens");
        }
    } catch (...) { return mfail(RMU_E_OOM, "rmu_bm25_search: out of memory while tokenising"); }

    Ctx& c = g_ctx;
    hipStream_t s = nullptr;
    std::shared_lock<std::shared_mutex> lk(h->mu);
    for (;;) {
        if (h->broken) return mfail(RMU_E_OOM, "rmu_bm25_search: an earlier add ran out of memory, the index is unusable");
        if (h->dl.empty()) {                     // nothing to search: no device work at all
            for (int64_t i = 0; i < nq * k; ++i) { out_scores[i] = -INFINITY; out_docs[i] = -1; }
            return RMU_OK;
        }
        if (!s) {
            if (c.ensure_stream() != RMU_OK) return mfail(RMU_E_HIP, "rmu_bm25_search: cannot create a stream");
            s = hip_stream ? (hipStream_t)hip_stream : c.stream;
        }
        if (!h->dirty) break;
        lk.unlock();
        {
            std::unique_lock<std::shared_mutex> wl(h->mu);
            if (h->dirty && !h->broken && !h->dl.empty()) {
                const int rc = build_image(h, s);
                if (rc != RMU_OK) { drop_image(h); return rc; }
            }
        }
        lk.lock();
    }

    // descriptors: term_ptr [nq + 1] | TermDesc [...], one pinned staging buffer, one copy
    size_t n_terms = 0;
    for (const auto& t : toks) n_terms += t.size();
    const size_t ptr_bytes = ((size_t)(nq + 1) * sizeof(u32) + 15) & ~(size_t)15;
    if (c.ensure_pin(ptr_bytes + (n_terms ? n_terms : 1) * sizeof(TermDesc)) != RMU_OK) return mfail(RMU_E_OOM, "rmu_bm25_search: pinned staging buffer");
    u32* tp = (u32*)c.pin;
    TermDesc* td = (TermDesc*)(c.pin + ptr_bytes);
    u32 nd = 0;
    try {
        for (int64_t i = 0; i < nq; ++i) {
            tp[i] = nd;
            for (const auto& tok : toks[i]) {
                const auto it = h->ids.find(tok);
                if (it == h->ids.end()) continue;                    // an unknown token contributes 0
                const u32 id = it->second;
                td[nd++] = TermDesc{h->post_ptr[id], (u32)(h->post_ptr[id + 1] - h->post_ptr[id]), h->weight[id]};
            }
        }
    } catch (...) { return mfail(RMU_E_OOM, "rmu_bm25_search: out of memory"); }
    tp[nq] = nd;
    const size_t stage_bytes = ptr_bytes + (size_t)nd * sizeof(TermDesc);

    // geometry.  Neither the tile nor the grid changes a bit of the result: both only spread the work
    const int64_t N = (int64_t)h->dl.size();
    int tile = (int)h->opt_tile;
    if (!tile) {
        tile = kMaxTile;
        while (tile > 1024 && ((N + tile - 1) / tile) * nq < 1024) tile >>= 1;
    }
    const int64_t tiles_total = (N + tile - 1) / tile;
    int64_t max_wgs = h->opt_max_wgs;
    if (!max_wgs) max_wgs = std::min<int64_t>(kMaxParts, std::max<int64_t>(8, 4096 / nq));
    const int64_t tiles_per_wg = (tiles_total + max_wgs - 1) / max_wgs;
    const int parts = (int)((tiles_total + tiles_per_wg - 1) / tiles_per_wg);
    if (tiles_per_wg * tile > 0x7FFFFFFFll) return mfail(RMU_E_INVALID, "rmu_bm25_search: document range of one workgroup too large");

    const size_t out_bytes = (size_t)nq * k * (sizeof(int64_t) + sizeof(float));
    BM25_TRY(c.stage.ensure(stage_bytes));
    BM25_TRY(c.partial.ensure((size_t)parts * nq * k * sizeof(u64)));
    BM25_TRY(c.out.ensure(out_bytes));
    BM25_TRY(hipMemcpyAsync(c.stage.p, c.pin, stage_bytes, hipMemcpyHostToDevice, s));
    Bm25Launch L{};
    L.post_doc = h->post_doc; L.post_tf = h->post_tf; L.doc_norm = h->doc_norm;
    L.term_ptr = (const u32*)c.stage.p;
    L.terms = (const TermDesc*)((const char*)c.stage.p + ptr_bytes);
    L.partial = (u64*)c.partial.p;
    L.n_docs = (u32)N; L.nq = (int)nq; L.k = k; L.tile = tile; L.tiles_per_wg = (int)tiles_per_wg;
    const dim3 grid((unsigned)parts, (unsigned)nq), block(kBlock);
    if (k <= 64) hipLaunchKernelGGL(bm25_topk_kernel<1>, grid, block, 0, s, L);
    else hipLaunchKernelGGL(bm25_topk_kernel<2>, grid, block, 0, s, L);
    BM25_TRY(hipGetLastError());
    int64_t* d_docs = (int64_t*)c.out.p;
    float* d_scores = (float*)((char*)c.out.p + (size_t)nq * k * sizeof(int64_t));
    const int rc = rmu_merge_final_launch((const u64*)c.partial.p, parts, nq, k, doc_base, 0, nullptr, d_scores, d_docs, nullptr, nullptr, s);
    if (rc != RMU_OK) { (void)hipStreamSynchronize(s); return mfail(rc, "rmu_bm25_search: merge launch failed"); }
    BM25_TRY(hipMemcpyAsync(out_docs, d_docs, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    BM25_TRY(hipMemcpyAsync(out_scores, d_scores, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, s));
    BM25_TRY(hipStreamSynchronize(s));
    return RMU_OK;
}
