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
// REMOVED DOCUMENTS (rmu.h, "Live documents"): every statistic (N, df, the vocabulary, avgdl) is the live corpus's.  A removal is host work
// (liveness bytes + one recount of df) and marks the image stale; the next search refreshes the weights, doc_norm and a liveness bitmap and
// leaves the postings where they are.  bm25_masked_kernel is bm25_topk_kernel with one more step: a document whose bit is clear selects with
// key 0.  rmu_bm25_search_subset launches the same kernel with allow AND live.  Out of scope: the ParadeDB SQL retriever.
//
// Host (plain C++, no HIP: testable without a GPU): whitespace tokenizer over a NUL-separated blob, term -> id map, per-term master posting
// vectors (ascending document id, tf) and dl.  Adding documents appends; document ids are insertion order.
// Device image, built lazily by the first search (one packed copy; the reference rebuilds its whole retriever per upload): post_doc[nnz] u32,
// post_tf[nnz] u32, doc_norm[N] fp32 = k1 * (1 - b + b * dl / avgdl) computed in double.  post_ptr[V + 1] and the fp32 term weights
// idf * (k1 + 1) stay on the host: a search resolves its terms there and ships (posting begin, length, weight) descriptors.
// ADDED DOCUMENTS: an add to a handle with a clean or stale image marks it GROWN.  New documents have the highest ids, so a term's new
// postings belong at the end of its list: the next search packs only those (the delta, O(V + new postings) on the host), uploads them with
// the old and the new post_ptr, and bm25_splice_kernel lays the new image out in HBM from the old image and the delta -- one pass, 8 bytes
// read and 8 written per posting; then the refresh step below recomputes weights, doc_norm and the bitmap, since N, df and avgdl moved for the
// old documents too.  RMU_BM25_OPT_REPACK_ON_ADD = 1 marks the image dirty instead (a full pack); the results are the same bit for bit.
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
//
// Kernel (bm25_groups_kernel, rmu_bm25_search_groups): the same body over a work table instead of a grid of equal ranges.  Every query has its
// own list of candidate documents; the host keeps, per list, only the tiles that hold a live candidate and turns runs of them into ranges
// (groups_plan), so the time follows the lists, not the postings of the terms over the whole corpus.  One workgroup per (query, range).
//
// Kernel (bm25_splice_kernel): a workgroup owns kSpliceSpan consecutive positions of the new image.  One binary search over the new post_ptr
// finds the term that holds its first position; from there every lane walks the terms forward as its positions (lane, lane + 256, ...) pass
// their ends.  Position j of term t is element j - new_ptr[t] of the term's list: the old image's while that is below the old length,
// the delta's after it.  The delta's pointer is not shipped: both arrays are prefix sums, so delta_ptr[t] = new_ptr[t] - old_ptr[t].
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rmu.h"
#include "rmu_common.h"
#include "rmu_host.h"

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
    const u32* mask;         // bm25_masked_kernel: bit d set = document d is a candidate; ceil(n_docs / 32) + 1 words.  bm25_groups_kernel: the
                             // mask words of all ranges, each range's at its GroupWork::mask_off
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

// The one body of all three kernels: query q over the documents [d_lo, d_hi), d_lo a multiple of the tile; the workgroup's sorted list goes to
// out[0, k).  MASKED: bit i of `mask` stands for document d_lo + i (2 * ceil((d_hi - d_lo) / 64) words are read); a document whose bit is clear
// gets key 0, the padding key the final merge turns into (-inf, -1); the score loop is the same, so a candidate's sum is the same ordered fp32
// sum whatever is masked and whatever the range.
template <int NPL, bool MASKED>
__device__ __forceinline__ void bm25_score_select(const Bm25Launch& p, const int q, const int64_t d_lo, const int64_t d_hi,
                                                  const u32* __restrict__ mask, u64* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float acc[kMaxTile];
    __shared__ u32 cur[kMaxTerms];
    __shared__ u32 wcnt[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u32 tb = p.term_ptr[q];
    const int nt = (int)(p.term_ptr[q + 1] - tb);
    const TermDesc* __restrict__ terms = p.terms + tb;

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
        // MASKED: lane i holds the two bitmap words of the wave's i-th 64-document batch of this tile (batch w + 4 * i; a tile has at most
        // 128 batches, 32 per wave), loaded here so that the term loop hides the latency.  t0 is a multiple of 64: the pair starts a word.
        u32 m_lo = 0, m_hi = 0;
        if constexpr (MASKED) {
            const int jb = (w + kWaves * lane) * 64;
            if (jb < cnt) {
                const u32* __restrict__ mp = mask + ((t0 - d_lo + jb) >> 5);
                m_lo = mp[0];
                m_hi = mp[1];
            }
        }
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
            u64 key = j < cnt ? rmu_make_key(acc[j], (u32)(t0 + j)) : 0ull;
            if constexpr (MASKED) {
                const int bi = j0 / kBlock;                                  // wave-uniform: the batch's words sit in lane bi
                const u32 lo = __shfl(m_lo, bi), hi = __shfl(m_hi, bi);
                if (!(((lane < 32 ? lo : hi) >> (lane & 31)) & 1u)) key = 0ull;
            }
            if (!__any(key > kth)) continue;                                 // (wave-uniform; a batch of masked documents never passes)
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
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        const int e = lane + 64 * i;
        if (e < p.k) out[e] = top[i];
    }
}

// grid = (workgroups over the document axis, queries): workgroup x owns tiles_per_wg tiles from its own offset, part list x of its query
template <int NPL, bool MASKED>
__device__ __forceinline__ void bm25_grid_range(const Bm25Launch& p) {
    const int q = blockIdx.y;
    const int64_t d_lo = (int64_t)blockIdx.x * p.tiles_per_wg * p.tile;
    const int64_t d_end = d_lo + (int64_t)p.tiles_per_wg * p.tile;
    const int64_t d_hi = d_end < (int64_t)p.n_docs ? d_end : (int64_t)p.n_docs;
    bm25_score_select<NPL, MASKED>(p, q, d_lo, d_hi, MASKED ? p.mask + (d_lo >> 5) : nullptr, p.partial + ((int64_t)blockIdx.x * p.nq + q) * p.k);
}
// every document is a candidate: what an index without removed documents launches for an unfiltered search
template <int NPL>
__global__ __launch_bounds__(kBlock) void bm25_topk_kernel(Bm25Launch p) { bm25_grid_range<NPL, false>(p); }
// candidates = the set bits of p.mask (the handle's liveness bitmap, or a call's allow AND live)
template <int NPL>
__global__ __launch_bounds__(kBlock) void bm25_masked_kernel(Bm25Launch p) { bm25_grid_range<NPL, true>(p); }

// rmu_bm25_search_groups: one workgroup per entry of a work table the host planned from the lists (groups_plan below).  An entry names its
// query, a document range that starts on a tile boundary and ends on one or at n_docs, the part list of the query it fills, and the first
// mask word of the range (allow AND live of the query's list; the queries of one list read the same words)
struct GroupWork {
    u32 q, part, d_lo, d_hi, mask_off;
};
static_assert(sizeof(GroupWork) == 20, "work table layout");
template <int NPL>
__global__ __launch_bounds__(kBlock) void bm25_groups_kernel(Bm25Launch p, const GroupWork* __restrict__ work) {
    const GroupWork g = work[blockIdx.x];
    bm25_score_select<NPL, true>(p, (int)g.q, (int64_t)g.d_lo, (int64_t)g.d_hi, p.mask + g.mask_off, p.partial + ((int64_t)g.part * p.nq + g.q) * p.k);
}

// ---- splice: old image + delta -> new image --------------------------------------------------------------------------------------------
constexpr int kSpliceItems = 8;                       // positions per lane
constexpr int kSpliceSpan = kBlock * kSpliceItems;    // positions per workgroup

struct SpliceLaunch {
    const u32* old_doc;      // the image so far: term t at [old_ptr[t], old_ptr[t + 1])
    const u32* old_tf;
    const u32* delta_doc;    // the postings of the documents added since: term t at [new_ptr[t] - old_ptr[t], new_ptr[t + 1] - old_ptr[t + 1])
    const u32* delta_tf;
    u32* new_doc;            // [nnz_new]
    u32* new_tf;
    const u64* old_ptr;      // [n_terms + 1]; a term that is new to the vocabulary has old length 0
    const u64* new_ptr;      // [n_terms + 1], new_ptr[n_terms] = nnz_new > 0
    u64 nnz_new;
    u32 n_terms;
};

__global__ __launch_bounds__(kBlock) void bm25_splice_kernel(SpliceLaunch p) {
    const u64 j0 = (u64)blockIdx.x * kSpliceSpan;          // < nnz_new: the grid is ceil(nnz_new / kSpliceSpan)
    // the only search: the last term t with new_ptr[t] <= j0, i.e. new_ptr[t] <= j0 < new_ptr[t + 1] (empty terms before it are passed over)
    u32 t = 0, hi = p.n_terms;                             // new_ptr[t] <= j0 < new_ptr[hi]
    while (hi - t > 1) {
        const u32 mid = t + ((hi - t) >> 1);
        if (p.new_ptr[mid] <= j0) t = mid;
        else hi = mid;
    }
    u64 b_new = p.new_ptr[t], e_new = p.new_ptr[t + 1], b_old = p.old_ptr[t], n_old = p.old_ptr[t + 1] - b_old;
#pragma unroll
    for (int i = 0; i < kSpliceItems; ++i) {
        const u64 j = j0 + (u64)(i * kBlock + (int)threadIdx.x);
        if (j >= p.nnz_new) break;
        if (e_new <= j) {                                  // j < nnz_new = new_ptr[n_terms]: the walk ends at a term below n_terms
            do {
                ++t;
                b_new = e_new;
                e_new = p.new_ptr[t + 1];
            } while (e_new <= j);
            b_old = p.old_ptr[t];
            n_old = p.old_ptr[t + 1] - b_old;
        }
        const u64 o = j - b_new;
        const bool from_old = o < n_old;
        const u64 src = from_old ? b_old + o : (b_new - b_old) + (o - n_old);
        p.new_doc[j] = (from_old ? p.old_doc : p.delta_doc)[src];
        p.new_tf[j] = (from_old ? p.old_tf : p.delta_tf)[src];
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

// per-thread stream and workspaces of rmu_bm25_search (every call drains its stream, so nothing of a thread's is ever in flight between calls)
struct Ctx {
    hipStream_t stream = nullptr;
    int device = -1;
    RmuDevBuf stage, partial, out;
    RmuPinBuf pin{4096};
    int ensure_stream() {
        rmu_follow_device(device);
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { stream = nullptr; return RMU_E_HIP; }
        return RMU_OK;
    }
    // only what has an order: the stream is drained and destroyed; the buffers free themselves behind this body
    ~Ctx() {
        if (rmu_runtime_down() || !stream) return;
        RMU_ENTRY();
        (void)hipStreamSynchronize(stream);
        (void)hipStreamDestroy(stream);
    }
};
thread_local Ctx g_ctx;

}  // namespace

struct rmu_bm25 {
    double k1 = 1.5, b = 0.75, epsilon = 0.25;
    std::unordered_map<std::string, u32> ids;      // term -> id, ids in order of first occurrence
    struct Postings { std::vector<u32> doc, tf; };
    std::vector<Postings> terms;                   // master posting vectors, ascending document id (removed documents' postings stay until compact)
    std::vector<u32> dl;
    uint64_t nnz = 0;                              // master postings
    // the live corpus: what every statistic and every score is computed from
    std::vector<uint8_t> live;                     // [N] 1 = live
    std::vector<u32> df;                           // [V] live documents that hold the term
    uint64_t n_live = 0, live_len = 0, live_nnz = 0, live_vocab = 0;
    bool broken = false;                           // an allocation failed half-way through an add
    int64_t opt_tile = 0, opt_max_wgs = 0, opt_repack_on_remove = 0, opt_repack_on_add = 0;
    // device image + the host half of it (valid while !dirty).  stale: the postings are in place but documents were removed since the
    // weights, doc_norm and the liveness bitmap were computed.  grown: the image holds the first imaged[t] master postings of every term
    // and documents were added since
    bool dirty = true, stale = false, grown = false;
    std::vector<u32> imaged;                       // [terms at the last pack or splice] master postings of the term the image has consumed
    uint64_t imaged_nnz = 0;                       // their sum
    uint64_t n_packs = 0, n_splices = 0, upload_bytes = 0;      // RMU_BM25_STAT_IMAGE_*
    u32* post_doc = nullptr;
    u32* post_tf = nullptr;
    float* doc_norm = nullptr;
    u32* live_bits = nullptr;                      // [ceil(N / 32) + 1], present while the image was built or refreshed with a removed document
    std::vector<u64> post_ptr;                     // [V + 1]
    std::vector<float> weight;                     // [V] fp32(idf * (k1 + 1)), 0 for a term no live document holds
    std::shared_mutex mu;
};

static void drop_image(rmu_bm25* h) {
    for (void* p : {(void*)h->post_doc, (void*)h->post_tf, (void*)h->doc_norm, (void*)h->live_bits})
        if (p) (void)rmu_free(p);
    h->post_doc = h->post_tf = h->live_bits = nullptr;
    h->doc_norm = nullptr;
    h->dirty = true;
    h->stale = h->grown = false;
}

// the one copy of the statistics -> (weights, doc_norm) step, over the live corpus: both the repack and the refresh path call it
static void live_weights_and_norms(const rmu_bm25* h, std::vector<float>& weight, std::vector<float>& norm) {
    const size_t V = h->terms.size(), N = h->dl.size();
    const double n = (double)h->n_live;
    std::vector<double> idf(V, 0.0);
    double idf_sum = 0.0;
    for (size_t t = 0; t < V; ++t) {
        if (!h->df[t]) continue;                   // not in the vocabulary of the live corpus
        const double df = (double)h->df[t];
        idf[t] = std::log(n - df + 0.5) - std::log(df + 0.5);
        idf_sum += idf[t];
    }
    const double repl = h->live_vocab ? h->epsilon * (idf_sum / (double)h->live_vocab) : 0.0;
    weight.assign(V, 0.f);
    for (size_t t = 0; t < V; ++t)
        if (h->df[t]) weight[t] = (float)((idf[t] < 0.0 ? repl : idf[t]) * (h->k1 + 1.0));
    const double avgdl = h->n_live ? (double)h->live_len / n : 0.0;
    norm.resize(N);
    for (size_t d = 0; d < N; ++d)
        norm[d] = (float)(h->k1 * (1.0 - h->b + (avgdl > 0.0 ? h->b * (double)h->dl[d] / avgdl : 0.0)));
}
// liveness bitmap [ceil(N / 32) + 1] (the kernel reads word pairs); `allow`: an ascending id list to AND with, or null
static void live_bitmap(const rmu_bm25* h, u32* words, const int64_t* allow, int64_t n_allow, int64_t* n_set) {
    const size_t N = h->dl.size(), nw = (N + 31) / 32 + 1;
    memset(words, 0, nw * sizeof(u32));
    int64_t set = 0;
    if (allow) {
        for (int64_t i = 0; i < n_allow; ++i)
            if (h->live[(size_t)allow[i]]) { words[allow[i] >> 5] |= 1u << (allow[i] & 31); ++set; }
    } else {
        for (size_t d = 0; d < N; ++d)
            if (h->live[d]) { words[d >> 5] |= 1u << (d & 31); ++set; }
    }
    if (n_set) *n_set = set;
}
static int upload_norms_and_bitmap(rmu_bm25* h, const std::vector<float>& norm, hipStream_t s) {
    const size_t N = h->dl.size(), nw = (N + 31) / 32 + 1;
    std::vector<u32> bits;
    if (N) RMU_HIP_TRY(hipMemcpyAsync(h->doc_norm, norm.data(), N * sizeof(float), hipMemcpyHostToDevice, s));
    if (h->n_live != N) {
        try { bits.resize(nw); } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_search: out of memory while packing the index"); }
        live_bitmap(h, bits.data(), nullptr, 0, nullptr);
        if (!h->live_bits) RMU_HIP_TRY(hipMalloc((void**)&h->live_bits, nw * sizeof(u32)));
        RMU_HIP_TRY(hipMemcpyAsync(h->live_bits, bits.data(), nw * sizeof(u32), hipMemcpyHostToDevice, s));
    }
    RMU_HIP_TRY(hipStreamSynchronize(s));             // (the host vectors are pageable and go out of scope)
    return RMU_OK;
}

// (exclusive lock held) pack the master vectors -- live documents' postings only -- and upload them; no search is in flight (see the header)
static int build_image(rmu_bm25* h, hipStream_t s) {
    drop_image(h);
    const size_t V = h->terms.size(), N = h->dl.size();
    const bool all_live = h->n_live == N;
    std::vector<u32> pk;          // post_doc | post_tf
    std::vector<float> norm;
    try {
        h->post_ptr.assign(V + 1, 0);
        h->imaged.resize(V);
        pk.resize(2 * (size_t)h->live_nnz);
        live_weights_and_norms(h, h->weight, norm);
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_search: out of memory while packing the index"); }
    u32* pdoc = pk.data();
    u32* ptf = pk.data() + h->live_nnz;
    u64 at = 0;
    for (size_t t = 0; t < V; ++t) {
        const auto& ps = h->terms[t];
        h->post_ptr[t] = at;
        h->imaged[t] = (u32)ps.doc.size();
        if (all_live) {
            if (!ps.doc.empty()) {
                memcpy(pdoc + at, ps.doc.data(), ps.doc.size() * sizeof(u32));
                memcpy(ptf + at, ps.tf.data(), ps.tf.size() * sizeof(u32));
            }
            at += ps.doc.size();
        } else {
            for (size_t i = 0; i < ps.doc.size(); ++i)
                if (h->live[ps.doc[i]]) { pdoc[at] = ps.doc[i]; ptf[at] = ps.tf[i]; ++at; }
        }
    }
    h->post_ptr[V] = at;
    if (at != h->live_nnz) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: internal error, the live posting count is out of step");
    const size_t pbytes = (size_t)h->live_nnz * sizeof(u32);
    RMU_HIP_TRY(hipMalloc((void**)&h->post_doc, pbytes ? pbytes : 4));
    RMU_HIP_TRY(hipMalloc((void**)&h->post_tf, pbytes ? pbytes : 4));
    RMU_HIP_TRY(hipMalloc((void**)&h->doc_norm, N ? N * sizeof(float) : 4));
    if (pbytes) {
        RMU_HIP_TRY(hipMemcpyAsync(h->post_doc, pdoc, pbytes, hipMemcpyHostToDevice, s));
        RMU_HIP_TRY(hipMemcpyAsync(h->post_tf, ptf, pbytes, hipMemcpyHostToDevice, s));
    }
    const int rc = upload_norms_and_bitmap(h, norm, s);
    if (rc != RMU_OK) return rc;
    h->imaged_nnz = h->nnz;
    ++h->n_packs;
    h->upload_bytes += 2 * pbytes;
    h->dirty = false;
    h->stale = false;
    return RMU_OK;
}

// (exclusive lock held, image clean but stale) the refresh path: documents were removed since the image was packed.  The postings stay as they
// are -- those of removed documents only ever touch accumulators the bitmap masks -- and the weights, doc_norm and the bitmap are recomputed.
static int refresh_image(rmu_bm25* h, hipStream_t s) {
    std::vector<float> norm;
    try {
        live_weights_and_norms(h, h->weight, norm);
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_search: out of memory while refreshing the index"); }
    const int rc = upload_norms_and_bitmap(h, norm, s);
    if (rc != RMU_OK) return rc;
    h->stale = false;
    return RMU_OK;
}

// (exclusive lock held, image grown, stale or not) the splice path.  The host touches only what is new: O(V) for the pointers and the master
// postings past imaged[t] of every term -- those of the documents added since, removed ones among them (the bitmap masks them, as it does on
// the refresh path).  Nothing of the handle changes before the new arrays are complete; any failure leaves it to the caller's drop_image.
static int splice_image(rmu_bm25* h, hipStream_t s) {
    const size_t V = h->terms.size(), V_old = h->imaged.size(), N = h->dl.size();
    const u64 nnz_old = h->post_ptr[V_old], nnz_delta = h->nnz - h->imaged_nnz, nnz_new = nnz_old + nnz_delta;
    std::vector<u64> old_ptr, new_ptr;
    std::vector<u32> dk;          // delta: post_doc | post_tf
    try {
        old_ptr.resize(V + 1);
        new_ptr.resize(V + 1);
        dk.resize(2 * (size_t)nnz_delta);
        h->imaged.resize(V, 0);
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_search: out of memory while packing the added documents"); }
    u32* ddoc = dk.data();
    u32* dtf = dk.data() + nnz_delta;
    u64 at = 0;                   // in the delta
    for (size_t t = 0; t < V; ++t) {
        const auto& ps = h->terms[t];
        old_ptr[t] = t < V_old ? h->post_ptr[t] : nnz_old;
        new_ptr[t] = old_ptr[t] + at;
        const size_t done = h->imaged[t], n = ps.doc.size() - done;
        if (n) {
            if (n > nnz_delta - at) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: internal error, the added posting count is out of step");
            memcpy(ddoc + at, ps.doc.data() + done, n * sizeof(u32));
            memcpy(dtf + at, ps.tf.data() + done, n * sizeof(u32));
            at += n;
        }
    }
    old_ptr[V] = nnz_old;
    new_ptr[V] = nnz_new;
    if (at != nnz_delta) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: internal error, the added posting count is out of step");

    struct Held {                 // device arrays that are not the handle's yet
        void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Held() { for (void* q : p) if (q) (void)rmu_free(q); }
    } held;
    void*& d_ptr = held.p[0]; void*& d_delta = held.p[1]; void*& d_doc = held.p[2]; void*& d_tf = held.p[3]; void*& d_norm = held.p[4];
    const size_t ptr_bytes = (V + 1) * sizeof(u64), delta_bytes = (size_t)nnz_delta * sizeof(u32), new_bytes = (size_t)nnz_new * sizeof(u32);
    RMU_HIP_TRY(hipMalloc(&d_ptr, 2 * ptr_bytes));
    RMU_HIP_TRY(hipMalloc(&d_delta, delta_bytes ? 2 * delta_bytes : 4));
    RMU_HIP_TRY(hipMalloc(&d_doc, new_bytes ? new_bytes : 4));
    RMU_HIP_TRY(hipMalloc(&d_tf, new_bytes ? new_bytes : 4));
    RMU_HIP_TRY(hipMalloc(&d_norm, N * sizeof(float)));
    if (nnz_new) {
        RMU_HIP_TRY(hipMemcpyAsync(d_ptr, old_ptr.data(), ptr_bytes, hipMemcpyHostToDevice, s));
        RMU_HIP_TRY(hipMemcpyAsync((char*)d_ptr + ptr_bytes, new_ptr.data(), ptr_bytes, hipMemcpyHostToDevice, s));
        if (delta_bytes) RMU_HIP_TRY(hipMemcpyAsync(d_delta, dk.data(), 2 * delta_bytes, hipMemcpyHostToDevice, s));
        const u64 wgs = (nnz_new + kSpliceSpan - 1) / kSpliceSpan;
        if (wgs > 0x7FFFFFFFull) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: too many postings for one splice launch");
        SpliceLaunch L{};
        L.old_doc = h->post_doc; L.old_tf = h->post_tf;
        L.delta_doc = (const u32*)d_delta; L.delta_tf = (const u32*)d_delta + nnz_delta;
        L.new_doc = (u32*)d_doc; L.new_tf = (u32*)d_tf;
        L.old_ptr = (const u64*)d_ptr; L.new_ptr = (const u64*)((const char*)d_ptr + ptr_bytes);
        L.nnz_new = nnz_new; L.n_terms = (u32)V;
        hipLaunchKernelGGL(bm25_splice_kernel, dim3((unsigned)wgs), dim3(kBlock), 0, s, L);
        RMU_HIP_TRY(hipGetLastError());
        RMU_HIP_TRY(hipStreamSynchronize(s));         // (the host vectors are pageable; the old arrays are free to go)
        h->upload_bytes += 2 * ptr_bytes + 2 * delta_bytes;
    }
    for (void* q : {(void*)h->post_doc, (void*)h->post_tf, (void*)h->doc_norm, (void*)h->live_bits})
        if (q) (void)rmu_free(q);
    h->post_doc = (u32*)d_doc; h->post_tf = (u32*)d_tf; h->doc_norm = (float*)d_norm;
    h->live_bits = nullptr;                        // (N grew: the refresh below allocates it again if a document is removed)
    d_doc = d_tf = d_norm = nullptr;
    h->post_ptr.swap(new_ptr);
    for (size_t t = 0; t < V; ++t) h->imaged[t] = (u32)h->terms[t].doc.size();
    h->imaged_nnz = h->nnz;
    h->grown = false;
    ++h->n_splices;
    return refresh_image(h, s);
}

extern "C" int rmu_bm25_create(rmu_bm25_t** out, double k1, double b, double epsilon) {
    RMU_ENTRY();
    if (!out) return rmu_fail(RMU_E_INVALID, "rmu_bm25_create: null argument");
    if (!(k1 >= 0.0) || !std::isfinite(k1) || !(b >= 0.0 && b <= 1.0) || !std::isfinite(epsilon))
        return rmu_fail(RMU_E_INVALID, "rmu_bm25_create: k1 must be finite and >= 0, b in [0, 1], epsilon finite");
    rmu_bm25* h = new (std::nothrow) rmu_bm25();
    if (!h) return rmu_fail(RMU_E_OOM, "rmu_bm25_create: out of memory");
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
    if (!h || n < 0 || bytes < n || (n > 0 && !blob)) return rmu_fail(RMU_E_INVALID, "rmu_bm25_add_texts: bad argument");
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (h->broken) return rmu_fail(RMU_E_OOM, "rmu_bm25_add_texts: an earlier add ran out of memory, the index is unusable");
    if ((uint64_t)h->dl.size() + (uint64_t)n > 0x7FFFFFFFull) return rmu_fail(RMU_E_INVALID, "rmu_bm25_add_texts: more than 2^31 - 1 documents");
    if (first_doc) *first_doc = (int64_t)h->dl.size();
    if (n == 0) {
        if (bytes != 0) return rmu_fail(RMU_E_INVALID, "rmu_bm25_add_texts: the blob does not hold exactly n NUL-terminated strings");
        return RMU_OK;
    }
    try {
        std::vector<std::pair<const char*, size_t>> docs;
        if (!split_blob(blob, bytes, n, docs)) return rmu_fail(RMU_E_INVALID, "rmu_bm25_add_texts: the blob does not hold exactly n NUL-terminated strings");
        if (h->dirty || h->opt_repack_on_add) h->dirty = true;
        else h->grown = true;                   // (clean or stale: the next search splices the new postings in)
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
                    h->df.push_back(0);
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
                ++h->live_nnz;
                if (h->df[seen[i]]++ == 0) ++h->live_vocab;
                i = j;
            }
            h->dl.push_back((u32)seen.size());
            h->live.push_back(1);
            ++h->n_live;
            h->live_len += seen.size();
        }
        h->broken = false;
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_add_texts: out of memory, the index is unusable"); }
    return RMU_OK;
}

extern "C" int rmu_bm25_stat(rmu_bm25_t* h, int what, double* out) {
    RMU_ENTRY();
    if (!h || !out) return rmu_fail(RMU_E_INVALID, "rmu_bm25_stat: null argument");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    switch (what) {
        case RMU_BM25_STAT_DOCS: *out = (double)h->dl.size(); break;
        case RMU_BM25_STAT_VOCAB: *out = (double)h->live_vocab; break;
        case RMU_BM25_STAT_NNZ: *out = (double)h->live_nnz; break;
        case RMU_BM25_STAT_AVGDL: *out = h->n_live ? (double)h->live_len / (double)h->n_live : 0.0; break;
        case RMU_BM25_STAT_LIVE_DOCS: *out = (double)h->n_live; break;
        case RMU_BM25_STAT_IMAGE_PACKS: *out = (double)h->n_packs; break;
        case RMU_BM25_STAT_IMAGE_SPLICES: *out = (double)h->n_splices; break;
        case RMU_BM25_STAT_IMAGE_UPLOAD_BYTES: *out = (double)h->upload_bytes; break;
        default: return rmu_fail(RMU_E_INVALID, "rmu_bm25_stat: unknown statistic");
    }
    return RMU_OK;
}

extern "C" int rmu_bm25_df(rmu_bm25_t* h, const char* term_utf8, int64_t* df) {
    RMU_ENTRY();
    if (!h || !term_utf8 || !df) return rmu_fail(RMU_E_INVALID, "rmu_bm25_df: null argument");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    try {
        const auto it = h->ids.find(term_utf8);
        *df = it == h->ids.end() ? 0 : (int64_t)h->df[it->second];
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_df: out of memory"); }
    return RMU_OK;
}

extern "C" int rmu_bm25_set_option(rmu_bm25_t* h, int option, int64_t value) {
    RMU_ENTRY();
    if (!h) return rmu_fail(RMU_E_INVALID, "rmu_bm25_set_option: null handle");
    std::unique_lock<std::shared_mutex> lk(h->mu);
    switch (option) {
        case RMU_BM25_OPT_TILE_DOCS:
            if (value != 0 && (value < 64 || value > kMaxTile || (value & (value - 1))))
                return rmu_fail(RMU_E_INVALID, "rmu_bm25_set_option: RMU_BM25_OPT_TILE_DOCS takes 0 or a power of two in [64, 8192]");
            h->opt_tile = value;
            break;
        case RMU_BM25_OPT_MAX_WGS:
            if (value < 0 || value > kMaxParts) return rmu_fail(RMU_E_INVALID, "rmu_bm25_set_option: RMU_BM25_OPT_MAX_WGS takes 0 .. 1024");
            h->opt_max_wgs = value;
            break;
        case RMU_BM25_OPT_REPACK_ON_REMOVE:
            if (value != 0 && value != 1) return rmu_fail(RMU_E_INVALID, "rmu_bm25_set_option: RMU_BM25_OPT_REPACK_ON_REMOVE takes 0 or 1");
            h->opt_repack_on_remove = value;
            break;
        case RMU_BM25_OPT_REPACK_ON_ADD:
            if (value != 0 && value != 1) return rmu_fail(RMU_E_INVALID, "rmu_bm25_set_option: RMU_BM25_OPT_REPACK_ON_ADD takes 0 or 1");
            h->opt_repack_on_add = value;
            break;
        default: return rmu_fail(RMU_E_INVALID, "rmu_bm25_set_option: unknown option");
    }
    return RMU_OK;
}

// ---- what rmu_bm25_search / _subset (search_enqueue) and rmu_bm25_search_groups (groups_impl) share: the queries' tokens, the image life
// cycle under the handle's lock, the term descriptors and the final merge ----------------------------------------------------------------
using QueryTokens = std::vector<std::vector<std::string>>;

// the limits of every search, then the tokens of each query
static int query_tokens(const char* query_blob, int64_t bytes, int64_t nq, int k, QueryTokens& toks) {
    if (nq < 1 || nq > 65535 || bytes < nq) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: 1 <= nq <= 65535 queries, each NUL-terminated");
    if (k < 1 || k > RMU_MAX_K) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: 1 <= k <= RMU_MAX_K");
    std::vector<std::pair<const char*, size_t>> qs;
    try {
        if (!split_blob(query_blob, bytes, nq, qs)) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: the blob does not hold exactly nq NUL-terminated strings");
        toks.resize((size_t)nq);
        for (int64_t i = 0; i < nq; ++i) {
            split_tokens(qs[i].first, qs[i].second, [&](const char* p, size_t len) { toks[i].emplace_back(p, len); });
            if (toks[i].size() > (size_t)kMaxTerms) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: a query has more than 1024 tokens");
        }
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_search: out of memory while tokenising"); }
    return RMU_OK;
}

// The image life cycle.  `lk` comes back holding the handle's shared lock over a clean image (not dirty, stale or grown) with *s_out the stream of
// the call -- or with *empty set: there is nothing to search and nothing was enqueued, no stream was even created.  check(&nothing) runs under
// the shared lock, the first time and AGAIN every time the lock was given up for a rebuild (documents may have been added meanwhile, never
// renumbered unseen): it validates what the call says about the documents and may set `nothing`.
template <class Check>
static int lock_clean_image(rmu_bm25_t* h, Ctx& c, uint64_t hip_stream, std::shared_lock<std::shared_mutex>& lk, hipStream_t* s_out, bool* empty,
                            Check check) {
    hipStream_t s = nullptr;
    *empty = false;
    lk = std::shared_lock<std::shared_mutex>(h->mu);
    for (;;) {
        if (h->broken) return rmu_fail(RMU_E_OOM, "rmu_bm25_search: an earlier add ran out of memory, the index is unusable");
        bool nothing = false;
        const int rc = check(&nothing);
        if (rc != RMU_OK) return rc;
        if (h->n_live == 0 || nothing) {         // nothing to search: no device work at all
            *empty = true;
            return RMU_OK;
        }
        if (!s) {
            if (c.ensure_stream() != RMU_OK) return rmu_fail(RMU_E_HIP, "rmu_bm25_search: cannot create a stream");
            s = hip_stream ? (hipStream_t)hip_stream : c.stream;
        }
        if (!h->dirty && !h->stale && !h->grown) break;
        lk.unlock();
        {
            std::unique_lock<std::shared_mutex> wl(h->mu);
            if (!h->broken && h->n_live != 0 && (h->dirty || h->stale || h->grown)) {
                const int rc2 = h->dirty ? build_image(h, s) : h->grown ? splice_image(h, s) : refresh_image(h, s);
                if (rc2 != RMU_OK) { drop_image(h); return rc2; }
            }
        }
        lk.lock();
    }
    *s_out = s;
    return RMU_OK;
}

// (shared lock held, image clean) term_ptr [nq + 1] | TermDesc [...] at the start of the thread's pinned buffer, which is made large enough
// for tail_bytes more behind them.  *ptr_bytes: where the descriptors start; *desc_bytes: where they end (a multiple of 16)
static int stage_terms(const rmu_bm25_t* h, Ctx& c, const QueryTokens& toks, size_t tail_bytes, size_t* ptr_bytes_out, size_t* desc_bytes_out) {
    const size_t nq = toks.size();
    size_t n_terms = 0;
    for (const auto& t : toks) n_terms += t.size();
    const size_t ptr_bytes = ((nq + 1) * sizeof(u32) + 15) & ~(size_t)15;
    if (c.pin.ensure(ptr_bytes + (n_terms ? n_terms : 1) * sizeof(TermDesc) + tail_bytes) != RMU_OK)
        return rmu_fail(RMU_E_OOM, "rmu_bm25_search: pinned staging buffer");
    u32* tp = (u32*)c.pin.p;
    TermDesc* td = (TermDesc*)(c.pin.p + ptr_bytes);
    u32 nd = 0;
    try {
        for (size_t i = 0; i < nq; ++i) {
            tp[i] = nd;
            for (const auto& tok : toks[i]) {
                const auto it = h->ids.find(tok);
                if (it == h->ids.end()) continue;                    // an unknown token contributes 0
                const u32 id = it->second;
                if (!h->df[id]) continue;                            // no live document holds it any more: like an unknown token
                td[nd++] = TermDesc{h->post_ptr[id], (u32)(h->post_ptr[id + 1] - h->post_ptr[id]), h->weight[id]};
            }
        }
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_search: out of memory"); }
    tp[nq] = nd;
    *ptr_bytes_out = ptr_bytes;
    *desc_bytes_out = ptr_bytes + (size_t)nd * sizeof(TermDesc);
    return RMU_OK;
}

// the launch parameters every kernel of the family reads, over the image and the staged descriptors
static Bm25Launch launch_params(const rmu_bm25_t* h, const Ctx& c, size_t ptr_bytes, int64_t nq, int k, int tile) {
    Bm25Launch L{};
    L.post_doc = h->post_doc; L.post_tf = h->post_tf; L.doc_norm = h->doc_norm;
    L.term_ptr = (const u32*)c.stage.p;
    L.terms = (const TermDesc*)((const char*)c.stage.p + ptr_bytes);
    L.partial = (u64*)c.partial.p;
    L.n_docs = (u32)h->dl.size(); L.nq = (int)nq; L.k = k; L.tile = tile;
    return L;
}

// behind the scoring launch: the part lists of c.partial -> *d_docs [nq, k] int64 (+ doc_base) and *d_scores [nq, k] fp32 in c.out
static int merge_parts(Ctx& c, int parts, int64_t nq, int k, int64_t doc_base, hipStream_t s, int64_t** d_docs_out, float** d_scores_out) {
    RMU_HIP_TRY(hipGetLastError());
    int64_t* d_docs = (int64_t*)c.out.p;
    float* d_scores = (float*)((char*)c.out.p + (size_t)nq * k * sizeof(int64_t));
    const int rc = rmu_merge_final_launch((const u64*)c.partial.p, parts, nq, k, doc_base, 0, nullptr, d_scores, d_docs, nullptr, nullptr, s);
    if (rc != RMU_OK) { (void)hipStreamSynchronize(s); return rmu_fail(rc, "rmu_bm25_search: merge launch failed"); }
    *d_docs_out = d_docs;
    *d_scores_out = d_scores;
    return RMU_OK;
}

// the default tile: the largest, halved while the launch would have fewer than 1024 workgroups (`tiles_at(tile)` of them)
template <class TilesAt>
static int pick_tile(const rmu_bm25_t* h, TilesAt tiles_at) {
    int tile = (int)h->opt_tile;
    if (!tile) {
        tile = kMaxTile;
        while (tile > 1024 && tiles_at(tile) < 1024) tile >>= 1;
    }
    return tile;
}
static int64_t pick_max_wgs(const rmu_bm25_t* h, int64_t nq) {
    return h->opt_max_wgs ? h->opt_max_wgs : std::min<int64_t>(kMaxParts, std::max<int64_t>(8, 4096 / nq));
}

// The first half of a search: everything up to and including the final merge is enqueued on *s_out (hip_stream, or the calling thread's own
// stream) and the results are left on the device, *d_docs [nq, k] int64 (+ doc_base) and *d_scores [nq, k] fp32, in the thread's workspace.  `lk`
// comes back holding the handle's shared lock, which the caller keeps until it has drained the stream (see the header: no reader is ever left in
// flight behind the lock).  *empty: there is nothing to search (every slot is (-inf, -1)) and nothing was enqueued.  expect_docs >= 0 (the hybrid
// call, rrf_fuse.hip): DOCS must equal it, checked under the lock before anything is enqueued.
static int search_enqueue(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, bool subset, const int64_t* docs,
                          int64_t n_sub, int64_t expect_docs, uint64_t hip_stream, std::shared_lock<std::shared_mutex>& lk, hipStream_t* s_out,
                          int64_t** d_docs_out, float** d_scores_out, bool* empty) {
    *empty = false;
    if (!h || !query_blob) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: null argument");
    QueryTokens toks;
    int rc = query_tokens(query_blob, bytes, nq, k, toks);
    if (rc != RMU_OK) return rc;

    Ctx& c = g_ctx;
    hipStream_t s = nullptr;
    rc = lock_clean_image(h, c, hip_stream, lk, &s, empty, [&](bool* nothing) {
        if (expect_docs >= 0 && (int64_t)h->dl.size() != expect_docs)
            return rmu_fail(RMU_E_INVALID, "rmu_hybrid_search: the sparse key table (" + std::to_string(expect_docs) + " keys) and the BM25 index (" +
                                            std::to_string(h->dl.size()) + " documents) are out of step");
        if (subset) {
            const int64_t n_docs = (int64_t)h->dl.size();
            for (int64_t i = 0; i < n_sub; ++i)
                if (docs[i] < 0 || docs[i] >= n_docs || (i > 0 && docs[i] <= docs[i - 1]))
                    return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_subset: docs must be strictly ascending document ids in [0, DOCS)");
            *nothing = n_sub == 0;
        }
        return (int)RMU_OK;
    });
    if (rc != RMU_OK || *empty) return rc;
    const int64_t N = (int64_t)h->dl.size();
    const bool masked = subset || h->n_live != (uint64_t)N;

    // descriptors: term_ptr [nq + 1] | TermDesc [...], one pinned staging buffer, one copy
    const size_t mask_bytes = subset ? (((size_t)N + 31) / 32 + 1) * sizeof(u32) : 0;      // allow AND live, behind the descriptors
    size_t ptr_bytes = 0, desc_bytes = 0;                                                   // (desc_bytes: a multiple of 16, the bitmap's word pairs are aligned)
    rc = stage_terms(h, c, toks, mask_bytes, &ptr_bytes, &desc_bytes);
    if (rc != RMU_OK) return rc;
    if (subset) {
        int64_t n_cand = 0;
        live_bitmap(h, (u32*)(c.pin.p + desc_bytes), docs, n_sub, &n_cand);
        if (n_cand == 0) { *empty = true; return RMU_OK; }
    }
    const size_t stage_bytes = desc_bytes + mask_bytes;

    // geometry.  Neither the tile nor the grid changes a bit of the result: both only spread the work
    const int tile = pick_tile(h, [&](int t) { return ((N + t - 1) / t) * nq; });
    const int64_t tiles_total = (N + tile - 1) / tile;
    const int64_t max_wgs = pick_max_wgs(h, nq);
    const int64_t tiles_per_wg = (tiles_total + max_wgs - 1) / max_wgs;
    const int parts = (int)((tiles_total + tiles_per_wg - 1) / tiles_per_wg);
    if (tiles_per_wg * tile > 0x7FFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: document range of one workgroup too large");

    const size_t out_bytes = (size_t)nq * k * (sizeof(int64_t) + sizeof(float));
    RMU_HIP_TRY(c.stage.ensure(stage_bytes));
    RMU_HIP_TRY(c.partial.ensure((size_t)parts * nq * k * sizeof(u64)));
    RMU_HIP_TRY(c.out.ensure(out_bytes));
    RMU_HIP_TRY(hipMemcpyAsync(c.stage.p, c.pin.p, stage_bytes, hipMemcpyHostToDevice, s));
    Bm25Launch L = launch_params(h, c, ptr_bytes, nq, k, tile);
    L.tiles_per_wg = (int)tiles_per_wg;
    L.mask = !masked ? nullptr : subset ? (const u32*)((const char*)c.stage.p + desc_bytes) : h->live_bits;
    const dim3 grid((unsigned)parts, (unsigned)nq), block(kBlock);
    if (!masked) {
        if (k <= 64) hipLaunchKernelGGL(bm25_topk_kernel<1>, grid, block, 0, s, L);
        else hipLaunchKernelGGL(bm25_topk_kernel<2>, grid, block, 0, s, L);
    } else {
        if (k <= 64) hipLaunchKernelGGL(bm25_masked_kernel<1>, grid, block, 0, s, L);
        else hipLaunchKernelGGL(bm25_masked_kernel<2>, grid, block, 0, s, L);
    }
    *s_out = s;
    return merge_parts(c, parts, nq, k, doc_base, s, d_docs_out, d_scores_out);
}

// ---- rmu_bm25_search_groups: the plan ------------------------------------------------------------------------------------------------------
// A pure host function of its arguments (exported for the tests as rmu_bm25_groups_plan_).  Per list that a query uses: the tiles that hold a
// live candidate; runs of consecutive kept tiles, cut into pieces of at most ceil(kept / cap) tiles so that a long list still spreads over the
// CUs; and, if that leaves more than `cap` pieces, every ceil(pieces / cap) neighbours joined into one range across the empty tiles between
// them (their mask words are zero).  A range is [first tile * tile, min(end of last tile, n_docs)) and owns 2 * ceil(length / 64) mask words:
// one bit per document plus what the kernel's word-pair load reads past the end.  The same pass checks every list, used or not: strictly
// ascending ids in [0, n_docs), RMU_E_INVALID otherwise.
namespace {
struct DocGroupsPlan {
    std::vector<u32> lo, hi, mask_off;      // the ranges of all lists, list after list
    std::vector<u32> first;                 // [n_lists + 1]: list g owns ranges first[g] .. first[g + 1] (none: unused, or no live candidate)
    int64_t n_work = 0, mask_words = 0, kept_tiles = 0;
    int max_parts = 0;
};
}  // namespace

static int groups_plan(int64_t n_docs, const uint8_t* live, int tile, int cap, const int64_t* docs, const int64_t* list_ptr, int n_lists,
                       const int32_t* q_list, int64_t nq, DocGroupsPlan& P) {
    try {
        std::vector<int64_t> users((size_t)n_lists, 0);
        for (int64_t i = 0; i < nq; ++i) ++users[(size_t)q_list[i]];
        P.first.assign((size_t)n_lists + 1, 0);
        std::vector<u32> kept, plo, phi;        // of one list: kept tiles; pieces [plo, phi) in tiles
        const int shift = __builtin_ctz((unsigned)tile);      // (the tile is a power of two)
        for (int g = 0; g < n_lists; ++g) {
            P.first[(size_t)g] = (u32)P.lo.size();
            kept.clear(); plo.clear(); phi.clear();
            const bool used = users[(size_t)g] != 0;
            int64_t prev = -1;
            for (int64_t i = list_ptr[g]; i < list_ptr[g + 1]; ++i) {
                const int64_t d = docs[i];
                if (d <= prev || d >= n_docs)               // (unused lists are checked all the same)
                    return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: every list must hold strictly ascending document ids in [0, DOCS)");
                prev = d;
                if (!used || !live[d]) continue;
                const u32 t = (u32)(d >> shift);
                if (kept.empty() || kept.back() != t) kept.push_back(t);
            }
            if (kept.empty()) continue;
            P.kept_tiles += (int64_t)kept.size();
            const size_t per = (kept.size() + (size_t)cap - 1) / (size_t)cap;
            for (const u32 t : kept) {
                if (!plo.empty() && phi.back() == t && phi.back() - plo.back() < per) ++phi.back();
                else { plo.push_back(t); phi.push_back(t + 1); }
            }
            const size_t join = (plo.size() + (size_t)cap - 1) / (size_t)cap;
            for (size_t a = 0; a < plo.size(); a += join) {
                const size_t b = std::min(plo.size(), a + join) - 1;
                const int64_t d_lo = (int64_t)plo[a] * tile, d_hi = std::min<int64_t>((int64_t)phi[b] * tile, n_docs);
                if (P.mask_words > 0x7FFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: the lists' tiles need more than 2^31 mask words");
                P.lo.push_back((u32)d_lo);
                P.hi.push_back((u32)d_hi);
                P.mask_off.push_back((u32)P.mask_words);
                P.mask_words += 2 * ((d_hi - d_lo + 63) / 64);
            }
            const int parts = (int)(P.lo.size() - P.first[(size_t)g]);
            P.max_parts = std::max(P.max_parts, parts);
            P.n_work += (int64_t)parts * users[(size_t)g];
        }
        P.first[(size_t)n_lists] = (u32)P.lo.size();
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_search_groups: out of memory while planning"); }
    return RMU_OK;
}
// the plan written out: work [P.n_work] in query order, part by part; mask [P.mask_words] = allow AND live of every range
static void groups_fill(const DocGroupsPlan& P, const uint8_t* live, const int64_t* docs, const int64_t* list_ptr, int n_lists, const int32_t* q_list,
                        int64_t nq, GroupWork* work, u32* mask) {
    memset(mask, 0, (size_t)P.mask_words * sizeof(u32));
    for (int g = 0; g < n_lists; ++g) {
        u32 r = P.first[(size_t)g];
        const u32 r_end = P.first[(size_t)g + 1];
        if (r == r_end) continue;
        for (int64_t i = list_ptr[g]; i < list_ptr[g + 1]; ++i) {
            const int64_t d = docs[i];
            if (!live[d]) continue;
            while ((int64_t)P.hi[r] <= d) ++r;          // (every live candidate lies in a range of its list: r stays below r_end)
            mask[P.mask_off[r] + (u32)((d - (int64_t)P.lo[r]) >> 5)] |= 1u << (d & 31);       // (lo is a multiple of 64)
        }
    }
    int64_t n = 0;
    for (int64_t i = 0; i < nq; ++i) {
        const size_t g = (size_t)q_list[i];
        for (u32 r = P.first[g]; r < P.first[g + 1]; ++r) work[n++] = GroupWork{(u32)i, r - P.first[g], P.lo[r], P.hi[r], P.mask_off[r]};
    }
}
// what does not depend on the index: the shape of list_ptr and q_list
static int groups_check_shape(const int64_t* list_ptr, int n_lists, const int32_t* q_list, int64_t nq) {
    if (n_lists < 1) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: n_lists >= 1");
    if (list_ptr[0] != 0) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: list_ptr[0] must be 0");
    for (int g = 0; g < n_lists; ++g)
        if (list_ptr[g + 1] < list_ptr[g]) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: list_ptr must be non-decreasing");
    for (int64_t i = 0; i < nq; ++i)
        if (q_list[i] < 0 || q_list[i] >= n_lists || (i > 0 && q_list[i] < q_list[i - 1]))
            return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: q_list must be non-decreasing list numbers in [0, n_lists)");
    return RMU_OK;
}

// Test hook (not in rmu.h): the plan for an index of n_docs documents with liveness bytes `live`.  out_work [work_cap, 5] int32 = (query, part,
// d_lo, d_hi, first mask word) per entry, out_mask [mask_cap] the mask words; counts[4] = entries, mask words, kept tiles, most parts of a
// query.  The lists are checked as the call checks them.  Entries or words beyond a capacity are not written (the counts still say how many).
extern "C" int rmu_bm25_groups_plan_(int64_t n_docs, const uint8_t* live, int tile, int cap, const int64_t* docs, const int64_t* list_ptr,
                                     int n_lists, const int32_t* q_list, int64_t nq, int32_t* out_work, int64_t work_cap, uint32_t* out_mask,
                                     int64_t mask_cap, int64_t* counts) {
    RMU_ENTRY();
    if (n_docs < 0 || n_docs > 0x7FFFFFFFll || (n_docs > 0 && !live) || !list_ptr || !q_list || !counts || nq < 1 || work_cap < 0 || mask_cap < 0 ||
        (work_cap > 0 && !out_work) || (mask_cap > 0 && !out_mask))
        return rmu_fail(RMU_E_INVALID, "rmu_bm25_groups_plan_: bad argument");
    if (tile < 64 || tile > kMaxTile || (tile & (tile - 1)) || cap < 1 || cap > kMaxParts)
        return rmu_fail(RMU_E_INVALID, "rmu_bm25_groups_plan_: tile is a power of two in [64, 8192], 1 <= cap <= 1024");
    int rc = groups_check_shape(list_ptr, n_lists, q_list, nq);
    if (rc != RMU_OK) return rc;
    if (list_ptr[n_lists] > 0 && !docs) return rmu_fail(RMU_E_INVALID, "rmu_bm25_groups_plan_: bad argument");
    DocGroupsPlan P;
    rc = groups_plan(n_docs, live, tile, cap, docs, list_ptr, n_lists, q_list, nq, P);
    if (rc != RMU_OK) return rc;
    counts[0] = P.n_work; counts[1] = P.mask_words; counts[2] = P.kept_tiles; counts[3] = P.max_parts;
    if (P.n_work <= work_cap && P.mask_words <= mask_cap) {
        try {
            std::vector<GroupWork> work((size_t)P.n_work + 1);
            std::vector<u32> mask((size_t)P.mask_words + 1);
            groups_fill(P, live, docs, list_ptr, n_lists, q_list, nq, work.data(), mask.data());
            static_assert(sizeof(GroupWork) == 5 * sizeof(int32_t), "one entry = five int32");
            if (P.n_work) memcpy(out_work, work.data(), (size_t)P.n_work * sizeof(GroupWork));
            if (P.mask_words) memcpy(out_mask, mask.data(), (size_t)P.mask_words * sizeof(u32));
        } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_groups_plan_: out of memory"); }
    }
    return RMU_OK;
}

// rmu_bm25_search_groups: the shared first half (tokens, life cycle, term descriptors), the plan, one launch over its work table, the merge
static int groups_impl(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, const int64_t* docs,
                       const int64_t* list_ptr, int n_lists, const int32_t* q_list, float* out_scores, int64_t* out_docs, uint64_t hip_stream) {
    if (!h || !query_blob || !list_ptr || !q_list || !out_scores || !out_docs) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: null argument");
    QueryTokens toks;
    int rc = query_tokens(query_blob, bytes, nq, k, toks);
    if (rc != RMU_OK) return rc;
    rc = groups_check_shape(list_ptr, n_lists, q_list, nq);
    if (rc != RMU_OK) return rc;
    if (list_ptr[n_lists] > 0 && !docs) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: null argument");

    Ctx& c = g_ctx;
    hipStream_t s = nullptr;
    bool empty = false;
    std::shared_lock<std::shared_mutex> lk;
    // the lists are checked and the plan is made in one pass over them, under the shared lock.  Geometry: the work follows the lists, so the
    // tile is sized by the tiles the queries' lists cover at least
    int64_t ids_of_queries = 0;
    for (int64_t i = 0; i < nq; ++i) ids_of_queries += list_ptr[q_list[i] + 1] - list_ptr[q_list[i]];
    DocGroupsPlan P;
    int tile = 0;
    rc = lock_clean_image(h, c, hip_stream, lk, &s, &empty, [&](bool* nothing) {
        P = DocGroupsPlan{};
        tile = pick_tile(h, [&](int t) { return ids_of_queries / t + nq; });
        const int prc = groups_plan((int64_t)h->dl.size(), h->live.data(), tile, (int)pick_max_wgs(h, nq), docs, list_ptr, n_lists, q_list, nq, P);
        *nothing = P.n_work == 0;                // no used list holds a live document
        return prc;
    });
    if (rc != RMU_OK) return rc;
    if (empty) {
        for (int64_t i = 0; i < nq * k; ++i) { out_scores[i] = -INFINITY; out_docs[i] = -1; }
        return RMU_OK;
    }
    if (P.n_work > 0x7FFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_groups: more than 2^31 - 1 workgroups; send fewer queries per call");

    // one pinned staging buffer, one copy: term_ptr | TermDesc [...] | mask words | work table
    const size_t mask_bytes = ((size_t)P.mask_words * sizeof(u32) + 15) & ~(size_t)15, work_bytes = (size_t)P.n_work * sizeof(GroupWork);
    size_t ptr_bytes = 0, desc_bytes = 0;
    rc = stage_terms(h, c, toks, mask_bytes + work_bytes, &ptr_bytes, &desc_bytes);
    if (rc != RMU_OK) return rc;
    groups_fill(P, h->live.data(), docs, list_ptr, n_lists, q_list, nq, (GroupWork*)(c.pin.p + desc_bytes + mask_bytes), (u32*)(c.pin.p + desc_bytes));
    const size_t stage_bytes = desc_bytes + mask_bytes + work_bytes, part_bytes = (size_t)P.max_parts * nq * k * sizeof(u64);
    RMU_HIP_TRY(c.stage.ensure(stage_bytes));
    RMU_HIP_TRY(c.partial.ensure(part_bytes));
    RMU_HIP_TRY(c.out.ensure((size_t)nq * k * (sizeof(int64_t) + sizeof(float))));
    RMU_HIP_TRY(hipMemcpyAsync(c.stage.p, c.pin.p, stage_bytes, hipMemcpyHostToDevice, s));
    RMU_HIP_TRY(hipMemsetAsync(c.partial.p, 0, part_bytes, s));          // key 0: a query with fewer ranges than the longest pads its part lists
    Bm25Launch L = launch_params(h, c, ptr_bytes, nq, k, tile);
    L.mask = (const u32*)((const char*)c.stage.p + desc_bytes);
    const GroupWork* work = (const GroupWork*)((const char*)c.stage.p + desc_bytes + mask_bytes);
    const dim3 grid((unsigned)P.n_work), block(kBlock);
    if (k <= 64) hipLaunchKernelGGL(bm25_groups_kernel<1>, grid, block, 0, s, L, work);
    else hipLaunchKernelGGL(bm25_groups_kernel<2>, grid, block, 0, s, L, work);
    int64_t* d_docs = nullptr;
    float* d_scores = nullptr;
    rc = merge_parts(c, P.max_parts, nq, k, doc_base, s, &d_docs, &d_scores);
    if (rc != RMU_OK) return rc;
    RMU_HIP_TRY(hipMemcpyAsync(out_docs, d_docs, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipMemcpyAsync(out_scores, d_scores, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    return RMU_OK;
}

// rmu_bm25_search (subset = false) and rmu_bm25_search_subset (candidates = the live documents of docs[0, n_sub)): the half above, then the
// copies to the caller's arrays and the one synchronisation
static int search_impl(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, bool subset, const int64_t* docs,
                       int64_t n_sub, float* out_scores, int64_t* out_docs, uint64_t hip_stream) {
    if (!h || !query_blob || !out_scores || !out_docs) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search: null argument");
    std::shared_lock<std::shared_mutex> lk;
    hipStream_t s = nullptr;
    int64_t* d_docs = nullptr;
    float* d_scores = nullptr;
    bool empty = false;
    const int rc = search_enqueue(h, query_blob, bytes, nq, k, doc_base, subset, docs, n_sub, -1, hip_stream, lk, &s, &d_docs, &d_scores, &empty);
    if (rc != RMU_OK) return rc;
    if (empty) {
        for (int64_t i = 0; i < nq * k; ++i) { out_scores[i] = -INFINITY; out_docs[i] = -1; }
        return RMU_OK;
    }
    RMU_HIP_TRY(hipMemcpyAsync(out_docs, d_docs, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipMemcpyAsync(out_scores, d_scores, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    return RMU_OK;
}

// rrf_fuse.hip (rmu_hybrid_search): the sparse member's list, left on the device on the caller's stream (rmu_common.h)
int rmu_bm25_search_enqueue_(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t expect_docs, hipStream_t stream,
                             std::shared_lock<std::shared_mutex>& lk, const int64_t** d_docs, bool* empty) {
    hipStream_t s = nullptr;
    int64_t* docs = nullptr;
    float* scores = nullptr;
    const int rc = search_enqueue(h, query_blob, bytes, nq, k, 0, false, nullptr, 0, expect_docs, (uint64_t)(uintptr_t)stream, lk, &s, &docs, &scores, empty);
    *d_docs = docs;
    return rc;
}

extern "C" int rmu_bm25_search(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, float* out_scores,
                               int64_t* out_docs, uint64_t hip_stream) {
    RMU_ENTRY();
    return search_impl(h, query_blob, bytes, nq, k, doc_base, false, nullptr, 0, out_scores, out_docs, hip_stream);
}

extern "C" int rmu_bm25_search_subset(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, const int64_t* docs,
                                      int64_t n_sub, float* out_scores, int64_t* out_docs, uint64_t hip_stream) {
    RMU_ENTRY();
    if (n_sub < 0 || (n_sub > 0 && !docs)) return rmu_fail(RMU_E_INVALID, "rmu_bm25_search_subset: bad document list");
    return search_impl(h, query_blob, bytes, nq, k, doc_base, true, docs, n_sub, out_scores, out_docs, hip_stream);
}

extern "C" int rmu_bm25_search_groups(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, const int64_t* docs,
                                      const int64_t* list_ptr, int n_lists, const int32_t* q_list, float* out_scores, int64_t* out_docs,
                                      uint64_t hip_stream) {
    RMU_ENTRY();
    return groups_impl(h, query_blob, bytes, nq, k, doc_base, docs, list_ptr, n_lists, q_list, out_scores, out_docs, hip_stream);
}

// ---- removal, compaction, persistence: host only -----------------------------------------------------------------------------------------
// (exclusive lock held) df, the live posting count and the live vocabulary from the master postings and the liveness bytes: one pass
static void recount_live(rmu_bm25* h) {
    h->live_nnz = 0;
    h->live_vocab = 0;
    const bool all_live = h->n_live == h->dl.size();
    for (size_t t = 0; t < h->terms.size(); ++t) {
        const auto& pd = h->terms[t].doc;
        u32 n = 0;
        if (all_live) n = (u32)pd.size();
        else
            for (const u32 d : pd) n += h->live[d];
        h->df[t] = n;
        h->live_nnz += n;
        h->live_vocab += n != 0;
    }
}

extern "C" int rmu_bm25_remove_docs(rmu_bm25_t* h, const int64_t* docs, int64_t n, int64_t* n_removed) {
    RMU_ENTRY();
    if (!h || n < 0 || (n > 0 && !docs)) return rmu_fail(RMU_E_INVALID, "rmu_bm25_remove_docs: bad argument");
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (h->broken) return rmu_fail(RMU_E_OOM, "rmu_bm25_remove_docs: an earlier add ran out of memory, the index is unusable");
    const int64_t N = (int64_t)h->dl.size();
    for (int64_t i = 0; i < n; ++i)
        if (docs[i] < 0 || docs[i] >= N) return rmu_fail(RMU_E_INVALID, "rmu_bm25_remove_docs: a document id is outside [0, DOCS)");
    int64_t removed = 0;
    for (int64_t i = 0; i < n; ++i) {
        const size_t d = (size_t)docs[i];
        if (!h->live[d]) continue;                 // already removed, or given twice
        h->live[d] = 0;
        --h->n_live;
        h->live_len -= h->dl[d];
        ++removed;
    }
    if (n_removed) *n_removed = removed;
    if (!removed) return RMU_OK;
    recount_live(h);
    if (h->opt_repack_on_remove) h->dirty = true;
    else h->stale = true;                          // (a dirty image stays dirty: the repack drops the postings anyway)
    return RMU_OK;
}

extern "C" int rmu_bm25_compact(rmu_bm25_t* h, int64_t* old_to_new, int64_t map_len, int64_t* n_after) {
    RMU_ENTRY();
    if (!h || !old_to_new) return rmu_fail(RMU_E_INVALID, "rmu_bm25_compact: null argument");
    std::unique_lock<std::shared_mutex> lk(h->mu);
    if (h->broken) return rmu_fail(RMU_E_OOM, "rmu_bm25_compact: an earlier add ran out of memory, the index is unusable");
    const size_t N = h->dl.size();
    if (map_len < (int64_t)N) return rmu_fail(RMU_E_INVALID, "rmu_bm25_compact: old_to_new holds fewer entries than the index has documents");
    u32 next = 0;
    for (size_t d = 0; d < N; ++d) old_to_new[d] = h->live[d] ? (int64_t)next++ : -1;
    for (int64_t d = (int64_t)N; d < map_len; ++d) old_to_new[d] = -1;
    if (n_after) *n_after = (int64_t)next;
    if (next == N) return RMU_OK;                  // nothing to reclaim: the image stays as it is
    for (auto& ps : h->terms) {                    // in place: an entry only ever moves towards the front
        size_t out = 0;
        for (size_t i = 0; i < ps.doc.size(); ++i)
            if (h->live[ps.doc[i]]) { ps.doc[out] = (u32)old_to_new[ps.doc[i]]; ps.tf[out] = ps.tf[i]; ++out; }
        ps.doc.resize(out);
        ps.tf.resize(out);
    }
    for (size_t d = 0; d < N; ++d)
        if (h->live[d]) h->dl[(size_t)old_to_new[d]] = h->dl[d];
    h->dl.resize(next);
    h->live.assign(next, 1);
    h->nnz = h->live_nnz;
    h->dirty = true;
    h->stale = false;
    return RMU_OK;
}

namespace {
// the index file: one flat little-endian file, in this order
//   "RMUBM25\0" | u32 version = 1 | u32 0 | f64 k1, b, epsilon | u64 N, V, nnz | u32 dl[N] | u8 live[N]
//   | V x (u32 length, bytes) terms in term-id order | u64 offsets[V + 1] | u32 posting documents[nnz] | u32 posting tfs[nnz]
constexpr char kMagic[8] = {'R', 'M', 'U', 'B', 'M', '2', '5', '\0'};
constexpr u32 kFileVersion = 1;
constexpr size_t kHeaderBytes = 8 + 8 + 3 * 8 + 3 * 8;
struct File {
    FILE* f = nullptr;
    ~File() { if (f) fclose(f); }
};
}  // namespace

extern "C" int rmu_bm25_save(rmu_bm25_t* h, const char* path) {
    RMU_ENTRY();
    if (!h || !path) return rmu_fail(RMU_E_INVALID, "rmu_bm25_save: null argument");
    std::shared_lock<std::shared_mutex> lk(h->mu);
    if (h->broken) return rmu_fail(RMU_E_OOM, "rmu_bm25_save: an earlier add ran out of memory, the index is unusable");
    File fl;
    fl.f = fopen(path, "wb");
    if (!fl.f) return rmu_fail(RMU_E_INVALID, std::string("rmu_bm25_save: cannot open ") + path + " for writing");
    bool ok = true;
    const auto put = [&](const void* p, size_t bytes) { if (bytes && fwrite(p, 1, bytes, fl.f) != bytes) ok = false; };
    const uint64_t N = h->dl.size(), V = h->terms.size();
    const u32 ver[2] = {kFileVersion, 0};
    const double par[3] = {h->k1, h->b, h->epsilon};
    const uint64_t cnt[3] = {N, V, h->nnz};
    put(kMagic, 8); put(ver, 8); put(par, 24); put(cnt, 24);
    put(h->dl.data(), N * sizeof(u32));
    put(h->live.data(), N);
    try {
        std::vector<const std::string*> names(V, nullptr);
        for (const auto& kv : h->ids) names[kv.second] = &kv.first;
        for (uint64_t t = 0; t < V; ++t) {
            const u32 len = (u32)names[t]->size();
            put(&len, 4);
            put(names[t]->data(), len);
        }
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_save: out of memory"); }
    uint64_t at = 0;
    for (uint64_t t = 0; t < V; ++t) { put(&at, 8); at += h->terms[t].doc.size(); }
    put(&at, 8);
    for (const auto& ps : h->terms) put(ps.doc.data(), ps.doc.size() * sizeof(u32));
    for (const auto& ps : h->terms) put(ps.tf.data(), ps.tf.size() * sizeof(u32));
    if (fflush(fl.f) != 0) ok = false;
    if (!ok) return rmu_fail(RMU_E_INVALID, std::string("rmu_bm25_save: writing ") + path + " failed");
    return RMU_OK;
}

extern "C" int rmu_bm25_load(rmu_bm25_t** out, const char* path) {
    RMU_ENTRY();
    if (!out || !path) return rmu_fail(RMU_E_INVALID, "rmu_bm25_load: null argument");
    const auto bad = [&](const char* what) { return rmu_fail(RMU_E_INVALID, std::string("rmu_bm25_load: ") + path + ": " + what); };
    File fl;
    fl.f = fopen(path, "rb");
    if (!fl.f) return bad("cannot open the file");
    if (fseek(fl.f, 0, SEEK_END) != 0) return bad("cannot seek");
    const long end = ftell(fl.f);
    if (end < 0 || fseek(fl.f, 0, SEEK_SET) != 0) return bad("cannot seek");
    const uint64_t size = (uint64_t)end;
    if (size < kHeaderBytes) return bad("shorter than the header");
    unsigned char head[kHeaderBytes];
    if (fread(head, 1, kHeaderBytes, fl.f) != kHeaderBytes) return bad("cannot read the header");
    u32 ver[2];
    double par[3];
    uint64_t cnt[3];
    memcpy(ver, head + 8, 8); memcpy(par, head + 16, 24); memcpy(cnt, head + 40, 24);
    if (memcmp(head, kMagic, 8) != 0 || ver[0] != kFileVersion) return bad("not a BM25 index file of this version");
    const double k1 = par[0], b = par[1], eps = par[2];
    if (!(k1 >= 0.0) || !std::isfinite(k1) || !(b >= 0.0 && b <= 1.0) || !std::isfinite(eps)) return bad("k1, b or epsilon out of range");
    const uint64_t N = cnt[0], V = cnt[1], nnz = cnt[2];
    // every size against the file's length BEFORE anything is allocated (each count first on its own: no product can overflow after that)
    if (N > 0x7FFFFFFFull || N > size || V > size || nnz > size) return bad("a count in the header exceeds the file's length");
    const uint64_t fixed = kHeaderBytes + 5 * N + 4 * V + 8 * (V + 1) + 8 * nnz;        // all but the terms' bytes
    if (fixed > size) return bad("the file is shorter than its header says");
    std::vector<char> buf;
    rmu_bm25* h = nullptr;
    try {
        buf.resize((size_t)(size - kHeaderBytes));
        if (fread(buf.data(), 1, buf.size(), fl.f) != buf.size()) return bad("cannot read the file");
        h = new rmu_bm25();
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_load: out of memory"); }
    struct Drop { rmu_bm25* h; ~Drop() { delete h; } } drop{h};
    h->k1 = k1; h->b = b; h->epsilon = eps;
    try {
        const char* p = buf.data();
        const char* e = p + buf.size();
        h->dl.resize((size_t)N);
        if (N) memcpy(h->dl.data(), p, (size_t)N * 4);
        p += N * 4;
        h->live.resize((size_t)N);
        if (N) memcpy(h->live.data(), p, (size_t)N);
        p += N;
        for (uint64_t d = 0; d < N; ++d) {
            if (h->live[d] > 1) return bad("a liveness byte is neither 0 nor 1");
            h->n_live += h->live[d];
            if (h->live[d]) h->live_len += h->dl[d];
        }
        h->terms.resize((size_t)V);
        h->df.assign((size_t)V, 0);
        const uint64_t tail = 8 * (V + 1) + 8 * nnz;
        for (uint64_t t = 0; t < V; ++t) {
            if ((uint64_t)(e - p) < 4 + tail) return bad("the terms run past the end of the file");
            u32 len;
            memcpy(&len, p, 4);
            p += 4;
            if (len == 0 || (uint64_t)len > (uint64_t)(e - p) || (uint64_t)(e - p) - len < tail) return bad("a term is empty or runs past the end of the file");
            if (!h->ids.emplace(std::string(p, len), (u32)t).second) return bad("a term occurs twice");
            p += len;
        }
        if ((uint64_t)(e - p) != tail) return bad("the file is longer or shorter than its header says");
        std::vector<uint64_t> off((size_t)V + 1);
        memcpy(off.data(), p, 8 * ((size_t)V + 1));
        p += 8 * (V + 1);
        if (off[0] != 0 || off[V] != nnz) return bad("the posting offsets do not cover the postings");
        for (uint64_t t = 0; t < V; ++t)
            if (off[t + 1] < off[t] || off[t + 1] > nnz) return bad("the posting offsets do not ascend");
        const char* pdoc = p;
        const char* ptf = p + 4 * nnz;
        std::vector<uint64_t> sum((size_t)N, 0);
        for (uint64_t t = 0; t < V; ++t) {
            const size_t n = (size_t)(off[t + 1] - off[t]);
            auto& ps = h->terms[t];
            ps.doc.resize(n);
            ps.tf.resize(n);
            if (n) {
                memcpy(ps.doc.data(), pdoc + 4 * off[t], 4 * n);
                memcpy(ps.tf.data(), ptf + 4 * off[t], 4 * n);
            }
            for (size_t i = 0; i < n; ++i) {
                if (ps.doc[i] >= N || (i > 0 && ps.doc[i] <= ps.doc[i - 1])) return bad("a term's postings do not ascend inside [0, N)");
                if (ps.tf[i] < 1) return bad("a posting has term frequency 0");
                sum[ps.doc[i]] += ps.tf[i];
            }
        }
        for (uint64_t d = 0; d < N; ++d)
            if (sum[d] != h->dl[d]) return bad("a document's length differs from the sum of its term frequencies");
        h->nnz = nnz;
        recount_live(h);
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_bm25_load: out of memory"); }
    drop.h = nullptr;
    *out = h;
    return RMU_OK;
}
