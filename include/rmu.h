/* rmu.h -- C-ABI of librmu.so: the MI355X-native retrieval hot path of RAGMeUp.
 *
 * The reference (AI-Commandos/RAGMeUp @ 2025-01-03) has no FFI for this path: its boundary is the
 * LangChain plug-in surface that server/RAGHelper.py touches.  librmu.so is what
 * OUR implementations of those plug-ins bind through ctypes; every entry point below names the
 * reference call it serves.  Plain pointers and sizes only -- no torch / C++ types cross this line.
 *
 * Conventions
 *   - return 0 = OK, <0 = error class (RMU_E_*); rmu_last_error() gives the thread-local message.
 *   - never throws; the caller owns every in/out buffer; the library owns what *_create made.
 *   - device pointers are plain HIP device addresses (e.g. torch.Tensor.data_ptr()).
 *   - hip_stream: 0 = an internal per-thread stream, results complete on return;
 *                 non-zero = a hipStream_t the work is ordered on (caller synchronises).  Scratch space belongs to the
 *                 calling THREAD: a call that returns with work in flight marks its end with an event, and the thread's
 *                 next call on any other stream (or stream 0) is ordered behind it -- consecutive calls from one thread
 *                 never overlap on the device, whichever streams they name; use one thread per concurrent stream.
 *   - thread-safe: searches on one index run concurrently (shared lock); add/remove are exclusive.
 *   - a good neighbour in the host process (the reference runs its LLM in PyTorch on the same GPU, RAGHelper_local.py:42-105): no entry point
 *     synchronises the whole device or issues a synchronous copy -- a writer (add that re-allocates, remove_rows, free) waits for exactly
 *     the streams on which searches of that index are still in flight -- and every entry point runs with the calling thread's stream-capture
 *     interaction mode set to relaxed for its duration, so a hipGraph / torch.cuda.graph capture on another thread is never invalidated.
 *   - row ids are int64 row numbers in insertion order; pk/metadata mapping stays in the host language.
 */
#ifndef RMU_H_
#define RMU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMU_OK 0
#define RMU_E_INVALID (-1) /* bad argument / unsupported shape */
#define RMU_E_HIP (-2)     /* HIP runtime error */
#define RMU_E_OOM (-3)     /* device or host allocation failed */
#define RMU_E_RCCL (-4)    /* RCCL error (librccl.so missing, communicator or collective failure) */

#define RMU_METRIC_IP 0     /* larger = better */
#define RMU_METRIC_COSINE 1 /* rows are stored L2-normalised, queries normalised per call */
#define RMU_METRIC_L2SQ 2   /* squared L2 distance on the stored (un-normalised) rows, smaller = better (Milvus "L2");
                             * dim <= 767 (rows carry -|x|^2 in one pad column: 384-d rows are stored 768 wide; at dim 384 the index also keeps the
                             * fp16 screening image and one fp32 norm per row).  There is no wide (dim > 767) L2 index. */

/* flags for rmu_index_search / rmu_topk_merge */
#define RMU_F_Q_DEVICE 1u   /* query pointer is a device address */
#define RMU_F_OUT_DEVICE 2u /* output pointers are device addresses */
#define RMU_F_SMALLER_BETTER 4u /* rmu_topk_merge / rmu_shard_allgather_topk: the scores are distances (RMU_METRIC_L2SQ lists) */

/* options for rmu_index_set_option */
#define RMU_OPT_SCREEN 1    /* 1 (default): searches may take the fp16 screening path; 0: always the exact fp32 scan.
                             * Results are identical either way (bench.py times both through this switch). */

#define RMU_OPT_SCREEN_MIN_NQ 2 /* n > 0: take the screening path for every batch of >= n queries whatever the corpus size (by
                             * default small batches over small corpora take the exact scan, which is faster there); 0: default.
                             * Results are identical either way (the tests force the path through this switch). */

#define RMU_OPT_LADDER_RATIO 3   /* tuning: growth ratio of the screening path's threshold ladder above 64k rows (0 = default: 3, or the
                             * small-batch default for <= 128 queries).  Results are identical for every value. */
#define RMU_OPT_LADDER_FIRST 4   /* tuning: rows of the ladder's smallest first range (0 = default).  Results identical for every value. */

#define RMU_OPT_SCREEN_BAND 7     /* tuning: 1 (default): the ladder's merges seed each launch's thresholds with max(K'-th best, k-th best - 2 EPS(q)),
                             * the lower edge of the sufficiency test's band; 0: with the K'-th best alone.  Results are identical either way. */

#define RMU_OPT_SCREEN_SPILL 8    /* tuning: 1 (default): in the seeded launches of the ladder (full batches: over 128 queries) a lane whose scores pass
                             * its threshold writes them out as they are and a sift kernel behind the launch files them (row ids, the query's
                             * threshold, the merge with the running candidates); 0: they are appended inside the scan's tile loop and merged,
                             * as before.  Results and re-run counts are identical either way. */
#define RMU_OPT_SCREEN_SPILL_CAP 9 /* tuning: records per spill list of RMU_OPT_SCREEN_SPILL (1..4096; 0 = default, 256).  A wave whose list is full
                             * goes on appending inside the tile loop; results are identical for every value (the tests force that path). */
#define RMU_OPT_SCREEN_REFRESH 10 /* tuning: 0 (default): in a spill launch of RMU_OPT_SCREEN_SPILL a wave re-reads its queries' shared thresholds only
                             * while it can use them -- at its first pair of tiles, once its spill list is full, and the wave that paces the
                             * workgroup; 1: every wave re-reads and refreshes them at every pair of tiles, as before.  Results and re-run
                             * counts are identical either way (0 is 1.3-1.5 % faster on the 10M x 1024 headline: profiles/screen_refresh.md). */

#define RMU_OPT_COMPACT_INPLACE 5 /* 0 (default): rmu_index_compact moves the rows into fresh, smaller allocations (in place when those do not
                             * fit); 1: always in place, the capacity stays.  Results are identical either way (the tests force the path). */

#define RMU_OPT_WIDE_SCAN 6 /* 0 (default) or 1.  1: an RMU_METRIC_IP / RMU_METRIC_COSINE index of ANY width sends its exact searches through
                             * scan_wide_kernel (the kernel of rows wider than RMU_MAX_DIM, which streams the queries) instead of the
                             * register-resident scan, and the screening path is off while it is set.  Results are identical either way, bit for
                             * bit (the tests compare the two kernels through this switch; tools/wide_probe.py times them side by side at 768).
                             * RMU_E_INVALID on an RMU_METRIC_L2SQ index. */

#define RMU_MAX_K 112       /* largest k the fused scan keeps in LDS */
#define RMU_MAX_DIM 768     /* widest row of the register-resident scans */
#define RMU_MAX_DIM_WIDE 3072 /* widest row of an index (RMU_METRIC_IP / RMU_METRIC_COSINE): rows of 769..3072 dimensions are padded to a multiple
                             * of 64 floats and searched by the exact fp32 scan that streams its queries (scan_wide.hip).  Everything works on
                             * such an index as on a narrow one -- add, reserve, remove_rows, compact, get_rows, mmr / search_mmr, save / load,
                             * caller streams, RMU_OPT_* (the screening and ladder options are accepted and change nothing) -- except:
                             *   - RMU_METRIC_L2SQ: dim <= 767 (rmu_index_create fails for a wide L2 index);
                             *   - rmu_index_search_subset, rmu_index_search_groups: rows of at most RMU_MAX_DIM dimensions (RMU_E_INVALID before anything is enqueued);
                             *   - rmu_bert_search_mmr: 384-d rows (the encoder's width), as ever;
                             *   - the fp16 screening path exists at dim 384 only. */

typedef struct rmu_index rmu_index_t;
typedef struct rmu_bert rmu_bert_t;
typedef struct rmu_comm rmu_comm_t;

/* ---- runtime ------------------------------------------------------------------------------- */
/* hipSetDevice(device_ordinal); idempotent.  Serves: RAGHelper_local.py:107-117 (device choice). */
int rmu_init(int device_ordinal);
const char* rmu_last_error(void);
/* "librmu <ver> gfx950" -- lets the host fail loudly on a wrong build. */
const char* rmu_version(void);

/* ---- HBM-resident flat index ------------------------------------------------------------------
 * dim in [1, RMU_MAX_DIM_WIDE] for RMU_METRIC_IP / RMU_METRIC_COSINE, [1, 767] for RMU_METRIC_L2SQ.  Rows are stored zero-padded to 192 / 384 /
 * 768 floats, wider ones to the next multiple of 64.
 * Serves: RAGHelper.py:385-404 (Milvus.from_documents / PGVector ctor -> an empty collection). */
int rmu_index_create(rmu_index_t** out, int dim, int metric, int64_t capacity_hint);
int rmu_index_free(rmu_index_t* idx);
int rmu_index_size(rmu_index_t* idx, int64_t* n_rows);
int rmu_index_dim(rmu_index_t* idx, int* dim);
int rmu_index_metric(rmu_index_t* idx, int* metric);
int rmu_index_set_option(rmu_index_t* idx, int option, int64_t value);
/* Bookkeeping a host may want to report (bench.py's indexing leg does): allocated row capacity, how often rmu_index_add had to
 * re-allocate and copy the corpus matrix (+ screening image) and the wall time that took, live (non-tombstoned) rows.
 * Serves: the growth of the Milvus collection under RAGHelper.py:423-434's 1000-document inserts (no capacity is known
 * up front there either). */
#define RMU_STAT_CAPACITY 1
#define RMU_STAT_GROW_COUNT 2
#define RMU_STAT_GROW_MS 3
#define RMU_STAT_LIVE_ROWS 4
#define RMU_STAT_COMPACT_COUNT 5  /* rmu_index_compact calls that dropped rows, and their wall time */
#define RMU_STAT_COMPACT_MS 6
int rmu_index_stat(rmu_index_t* idx, int what, double* out);
/* Make room for `rows` rows in all (grow-only; at most ONE re-allocation, none if the capacity is there).  A re-allocation waits for
 * everything in flight on the device before the old matrix is freed: a caller that knows how many rows are coming -- or that is about to
 * leave work in flight (the insert pipeline's worker, between two forwards) -- pays for it at a moment of its choosing instead of inside
 * an rmu_index_add behind a forward.  Serves: RAGHelper.py:423-434's insert loop (the collection grows batch by batch). */
int rmu_index_reserve(rmu_index_t* idx, int64_t rows);

/* Append n rows ([n, dim] fp32 row-major, host or device).  *first_row = row id of vecs[0].
 * Serves: RAGHelper.py:431, :525 (db.add_documents -> add_texts -> insert). */
int rmu_index_add(rmu_index_t* idx, const float* vecs, int64_t n, int is_device, int64_t* first_row);

/* Tombstone rows (they stop appearing in results; their storage stays until rmu_index_compact).  *n_removed counts rows
 * that were live.  Serves: server.py:373-377 (collection.delete('source == ...') -> delete_count). */
int rmu_index_remove_rows(rmu_index_t* idx, const int64_t* rows, int64_t n, int64_t* n_removed);

/* Drop every tombstoned row: live rows keep their relative order and are renumbered 0..n_live-1.  old_to_new (host, may be
 * NULL) receives map_len >= n entries: the new id of old row r, or -1 if r was dead (entries [n, map_len) are set to -1; the map is
 * valid when the call returns 0).  *n_after = rows after the call.  map_len < n -> RMU_E_INVALID and nothing changes: read n with
 * rmu_index_size first, and expect an add from another thread to land in between.
 * Storage: by default each array (fp32 rows, fp16 screening image, L2 norms) moves into a new allocation of
 * max(4096, n_live + n_live / 8 + 1024) rows, one array at a time (the old one is freed before the next is allocated); in place, with the
 * capacity kept, under RMU_OPT_COMPACT_INPLACE, when that capacity would not be smaller, or when an allocation fails (RMU_E_OOM, index
 * unchanged, only when not even the in-place path's 64 MiB staging buffer fits; should that happen after the matrix has moved, the
 * screening image is dropped instead, as after a growth without room for it).  No dead row: nothing moves.  Results of every search
 * afterwards equal those before it with the row ids mapped.
 * Searches of the index wait (exclusive lock) and scans still in flight on callers' streams are waited for first, as for growth.
 * Serves: server.py:353-385 + RAGHelper.py:518-538 (delete / re-upload cycle). */
int rmu_index_compact(rmu_index_t* idx, int64_t* old_to_new, int64_t map_len, int64_t* n_after);

/* Gather stored rows to the host ([n, dim] fp32).  Serves: the MMR retriever's
 * `col.query(expr="pk in [...]", output_fields=[vector])` round trip (RAGHelper.py:497-499). */
int rmu_index_get_rows(rmu_index_t* idx, const int64_t* rows, int64_t n, float* out_host);

/* Batched greedy maximal-marginal-relevance selection on the device (fp64, one wave per query): for query i pick k of the
 * fetch_k candidate rows rows[i, :] (index-local ids as rmu_index_search returned them, -1 = absent): first the candidate
 * most similar to the query, then repeatedly argmax lambda*cos(q,x) - (1-lambda)*max cos(x, picked), lowest position on
 * ties.  out_pos [nq, k] int32 = positions in the candidate list (-1 past the number of candidates).
 * An id that is not a row of the index (>= its size) and the id of a REMOVED row (a stale list: search, remove_rows, then mmr) are absent
 * as well: never picked, not counted as candidates, and the output is padded with -1 accordingly.  (Both kernels decide this by the
 * row's norm -- a removed row is NaN -- so a live row that holds a NaN is absent too.)
 * flags: RMU_F_Q_DEVICE (q), RMU_F_OUT_DEVICE (rows and out_pos).  fetch_k <= 64.
 * Serves: VectorStoreRetriever(search_type="mmr") -> maximal_marginal_relevance (RAGHelper.py:497-499) without the
 * per-query "fetch 20 vectors by pk" round trip. */
int rmu_index_mmr(rmu_index_t* idx, const float* q, int64_t nq, const int64_t* rows, int fetch_k, int k,
                  double lambda_mult, unsigned flags, int32_t* out_pos);

/* The reference's per-request retrieval in ONE call (VectorStoreRetriever.invoke with search_type="mmr", RAGHelper.py:497-499:
 * dense top-fetch_k, then maximal_marginal_relevance over those candidates): rmu_index_search followed by rmu_index_mmr on
 * the device-resident candidate list, one host round trip.  HOST q [nq, dim]; HOST outputs out_rows [nq, k] int64 (row ids +
 * row_base in pick order, -1 past the number of candidates) and out_scores [nq, k] fp32 (the search score of each pick; may
 * be NULL).  fetch_k <= 64, k <= fetch_k.  Results equal rmu_index_search + rmu_index_mmr called one after the other. */
int rmu_index_search_mmr(rmu_index_t* idx, const float* q, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t row_base,
                         int64_t* out_rows, float* out_scores);

/* Persist / restore the corpus matrix (flat file: 64-byte header, liveness bytes, fp32 rows; restart = one H2D copy).
 * Serves: the Milvus-Lite `data.db` the reference re-opens when vector_store_initial_load is False
 * (RAGHelper.py:391, :417; .env.template:33,36).  Tombstones survive (poisoned rows are stored as they are). */
int rmu_index_save(rmu_index_t* idx, const char* path);
int rmu_index_load(rmu_index_t** out, const char* path);

/* Exact top-k of every query against all live rows (dim 384, k <= 104, any metric: fp16 screening + exact fp32 re-score under a
 * per-query sufficiency test; otherwise, and for every query that fails the test, the exact fp32 fused scan -- the
 * returned ids and scores are those of the exact scan either way; the failing queries are re-run by launches that are
 * predicated on the device, so the call never waits on the host for a decision and, given a caller stream with device
 * buffers and nq <= 8192, returns without synchronising it).
 *   q [nq, dim] fp32; out_scores [nq, k] fp32, out_rows [nq, k] int64, best first,
 *   order (score, then lower row id); slots beyond the live row count hold (-inf | +inf for L2SQ, -1).
 *   row_base is added to every returned row id (shard offset).
 * Serves: RAGHelper.py:497-499 -> vector-store similarity search (Milvus col.search FLAT). */
int rmu_index_search(rmu_index_t* idx, const float* q, int64_t nq, int k, unsigned flags,
                     int64_t row_base, float* out_scores, int64_t* out_rows, uint64_t hip_stream);

/* Exact top-k of every query against the rows ONE list names (the same list for all nq queries), in time proportional to the list,
 * not the corpus: a gathered form of the exact fp32 scan (no copy of the subset is made).  rows [n_sub] int64: strictly ascending
 * index-local row ids.  A HOST list is checked before anything is enqueued (not ascending, negative or >= n -> RMU_E_INVALID, nothing
 * launched) and copied; a DEVICE list (RMU_F_ROWS_DEVICE) is the caller's contract: ids outside [0, n) are ignored.  Tombstoned rows
 * in the list never appear.  Everything else -- q, k, row_base, flags, output format and order (score, then lower row id), the stream
 * contract -- is rmu_index_search's, and every returned score has the bits rmu_index_search returns for that row.  n_sub == 0, or fewer
 * than k live rows in the list: the remaining slots hold (-inf | +inf for L2SQ, -1).
 * The index must hold rows of at most RMU_MAX_DIM dimensions: on a wider one the call returns RMU_E_INVALID before anything is enqueued (the
 * gathered form of the wide scan does not exist yet).
 * Serves: VectorStore.similarity_search(**kwargs) with a filter -- Milvus col.search(expr='source == "a.pdf"') / PGVector
 * filter={"source": "a.pdf"} behind the retriever's search_kwargs (RAGHelper.py:497-499). */
#define RMU_F_ROWS_DEVICE 8u   /* rmu_index_search_subset, rmu_index_search_groups: `rows` is a device address */
int rmu_index_search_subset(rmu_index_t* idx, const float* q, int64_t nq, int k, unsigned flags, int64_t row_base,
                            const int64_t* rows, int64_t n_sub, float* out_scores, int64_t* out_rows, uint64_t hip_stream);

/* rmu_index_search_subset with ONE LIST PER GROUP OF QUERIES, in one call: many concurrent requests, each filtered to its own rows, share
 * one scan.  rows = n_lists lists laid end to end, list g = rows[list_ptr[g] .. list_ptr[g + 1]) (list_ptr[0] = 0), each strictly
 * ascending index-local row ids; lists may overlap, repeat each other, be empty or go unused.  q_list[i] in [0, n_lists) = the list of
 * query i; it must be NON-DECREASING, so that the queries of a list are adjacent (the caller reorders its queries, the library does not).
 * list_ptr [n_lists + 1] and q_list [nq] are always HOST arrays (the plan is made from them); rows is a host array, or a device array
 * with RMU_F_ROWS_DEVICE.  Host lists are checked as rmu_index_search_subset checks its list, before anything is enqueued; device lists
 * are the caller's contract: ids outside [0, n) are ignored.
 * Result of query i: exactly what rmu_index_search_subset(idx, q_i, 1, k, ..., list q_list[i]) returns -- the same order (score, then
 * lower row id), the same (-inf | +inf for L2SQ, -1) padding, no tombstoned row, every score with the bits rmu_index_search gives that
 * row (the two scans run one tile loop).  RMU_F_Q_DEVICE, RMU_F_OUT_DEVICE and row_base as there.
 * Limits (RMU_E_INVALID with a message, before anything is enqueued): 1 <= nq <= 8192 (more queries: more calls), 1 <= k <= RMU_MAX_K,
 * n_lists >= 1, the lists together and the index each hold fewer than 2^32 rows, rows of at most RMU_MAX_DIM dimensions (a wide index is
 * refused, as by rmu_index_search_subset).
 * Work: at most two scan launches however many lists there are (one per geometry of the gathered scan), one merge, one row-id pass.
 * The call ALWAYS drains its stream, caller stream and device buffers included: its work table travels through the calling thread's
 * pinned workspace, as rmu_attribution's group table does.
 * Serves: the same filtered retrieval (RAGHelper.py:497-499 with search_kwargs) for a BATCH of requests whose filters differ -- every
 * user asking about their own upload, expr='source == "<their file>"' -- which the reference answers one col.search per request. */
int rmu_index_search_groups(rmu_index_t* idx, const float* q, int64_t nq, int k, unsigned flags, int64_t row_base,
                            const int64_t* rows, const int64_t* list_ptr, int n_lists, const int32_t* q_list,
                            float* out_scores, int64_t* out_rows, uint64_t hip_stream);

/* Merge `parts` per-shard top-k lists ([parts, nq, k] each, best first; larger score = better unless
 * RMU_F_SMALLER_BETTER) into one [nq, k].  Ties: lower part index first (give shards in ascending row order).
 * Serves: the 8-GPU shard merge after the RCCL all-gather; no reference counterpart. */
int rmu_topk_merge(const float* scores, const int64_t* rows, int parts, int64_t nq, int k,
                   unsigned flags, float* out_scores, int64_t* out_rows, uint64_t hip_stream);

/* ---- multi-GPU: the one exchange step of the row-sharded search -----------------------------------------
 * One process per GPU.  Rank 0 calls rmu_comm_unique_id and hands the 128 bytes to the other ranks by any side channel
 * (a file, a socket, torch.distributed's store); every rank then calls rmu_comm_init on ITS device (rmu_init first).
 * RCCL is bound at run time (dlopen of librccl.so; RMU_E_RCCL if absent).  No reference counterpart. */
#define RMU_COMM_ID_BYTES 128
int rmu_comm_unique_id(void* id_out /* RMU_COMM_ID_BYTES */);
int rmu_comm_init(rmu_comm_t** out, const void* id, int world, int rank);
int rmu_comm_free(rmu_comm_t* comm);
int rmu_comm_world(rmu_comm_t* comm, int* world, int* rank);
/* Every rank passes its local [nq, k] lists (what rmu_index_search returned with row_base = the shard's first row):
 * ONE RCCL all-gather of nq*k*12 bytes per rank over xGMI, then the W lists are merged on the device; every rank ends
 * with the same global [nq, k].  flags: RMU_F_Q_DEVICE (inputs), RMU_F_OUT_DEVICE (outputs), RMU_F_SMALLER_BETTER. */
int rmu_shard_allgather_topk(rmu_comm_t* comm, const float* scores, const int64_t* rows, int64_t nq, int k, unsigned flags,
                             float* out_scores, int64_t* out_rows, uint64_t hip_stream);

/* Test hook (tests/test_search_gpu.py), not a product entry point: the screening pass's K' = 32 candidates of each of nq
 * host queries -- approximate scores, row ids, the exact fp32 score of the same rows, and the error bound EPS(q) of the
 * sufficiency test -- so |approx - exact| <= EPS can be checked on the hardware.  All outputs are host arrays
 * ([nq, 32] x 3 and [nq]); absent candidates are (-inf, -1, -inf). */
int rmu_index_screen_candidates(rmu_index_t* idx, const float* q_host, int64_t nq, float* out_approx, int64_t* out_rows,
                                float* out_exact, float* out_eps);

/* Timing hook for bench.py: duration in ms of the last fused scan kernel launched by the calling
 * thread, measured with hipEvents on the stream the kernel ran on; <0 if none. */
float rmu_last_scan_ms(void);
/* Same for the whole search (scan + merge), and the launch geometry of the last scan. */
float rmu_last_search_ms(void);
int rmu_last_scan_geometry(int* grid, int* block, int* lds_bytes, int* passes);
/* How the calling thread's last rmu_index_search was answered: >0 by the fp16 screening ladder + exact fp32 re-score;
 * <0 the same, with that many queries failing the sufficiency test and re-run on the exact fp32 scan (patched in; the
 * count is known only when the call itself drained the stream, i.e. not for an un-synchronised caller stream);
 * 0 by the exact fp32 scan alone.  Results are identical in all three cases. */
int rmu_last_screened(void);
/* Enable (1) / disable (0) the event timing above for the calling thread (off by default). */
int rmu_set_timing(int on);
/* Diagnostic for bench.py (no reference counterpart): the rate in TFLOP/s THIS GPU sustains on v_mfma_f32_32x32x16 with operands that change
 * from instruction to instruction (random N(0, 3.3) values: the fp16 image's distribution) -- the power-limited roof a kernel working on data
 * can approach, as opposed to the nominal peak reached on constant operands (tools/ubench/mfma_power.hip, profiles/r06_mfma_power.txt).
 * dtype 0 = f16, 1 = bf16.  variant 0 = nothing but MFMAs (two waves per SIMD on every CU); variant 1 (f16 only) = the screening kernel's operand
 * delivery beside them: one 1-KiB LDS fragment read per MFMA + one 1-KiB LDS-DMA piece per wave and 8 MFMAs.  Runs ~millis ms of back-to-back
 * launches on a stream of its own and returns the mean of the last half of them.  Thread-safe; allocates and frees its own buffers. */
int rmu_probe_mfma_rate(int dtype, int variant, int millis, double* tflops_out);

/* ---- BERT encoder (bi-encoder and cross-encoder forwards) -------------------------------------
 * Serves: HuggingFaceEmbeddings.embed_documents / embed_query (RAGHelper_local.py:107-117 via
 * RAGHelper.py:423-434) and HuggingFaceCrossEncoder.score (RAGHelper.py:483-486 ->
 * ScoredCrossEncoderReranker.py:42).
 * Two geometries are built (post-LayerNorm BERT, GELU(erf), absolute positions, 1 <= layers <= 48, max_pos <= 512):
 *   TUNED    hidden 384, 12 heads of 32, ffn 1536 (the MiniLM / bge-small family): its own kernels, every entry point below;
 *   GENERAL  64-wide heads: hidden = 64 * heads with 2 <= heads <= 16 (128 .. 1024: bert-tiny .. bert-base / bge-base 768/12/3072 ..
 *            bert-large / bge-large 1024/16/4096), ffn a multiple of 64 in [64, 4096] (csrc/bert_any.hip).  Served by rmu_bert_encode
 *            in all four modes; rmu_bert_encode_host, rmu_bert_search_mmr, rmu_bert_search_hybrid, rmu_bert_attribute and
 *            rmu_bert_rerank need the tuned geometry and return RMU_E_INVALID for such a model (before any device work).
 * Anything else -- another head width, hidden above 1024, ffn above 4096 -- is refused by rmu_bert_create. */
typedef struct rmu_bert_cfg {
    int vocab_size;   /* 30522 */
    int hidden;       /* 384, or 64 * heads (128 .. 1024) */
    int layers;       /* 6 (1 .. 48) */
    int heads;        /* 12 at hidden 384 (head_dim 32); 2 .. 16 otherwise (head_dim 64) */
    int ffn;          /* 1536 at hidden 384; a multiple of 64 up to 4096 otherwise */
    int max_pos;      /* 512 */
    int type_vocab;   /* 2 */
    float ln_eps;     /* 1e-12 */
    int has_head;     /* 1: pooler.dense + classifier (cross-encoder) weights are supplied */
} rmu_bert_cfg;

/* weights: array of DEVICE pointers to fp32 tensors in HF layout, order documented in
 * ragmeup_amd/bert.py (WEIGHT_ORDER).  The library converts them to bf16 MFMA operand layout once. */
int rmu_bert_create(rmu_bert_t** out, const rmu_bert_cfg* cfg, const void* const* weight_ptrs, int n_weights);
int rmu_bert_free(rmu_bert_t* m);
/* What rmu_bert_encode writes (`mode`): the head behind the transformer as the checkpoint declares it --
 * sentence-transformers `1_Pooling/config.json` (pooling_mode_mean_tokens | pooling_mode_cls_token) and `modules.json`
 * (Normalize present or not) for the bi-encoder, BertForSequenceClassification(num_labels = 1) for the cross-encoder. */
#define RMU_BERT_POOL_MEAN 0   /* masked mean over the tokens (+ L2 normalise) -> out_dev fp32 [batch, out_stride] (first `hidden` cols) */
#define RMU_BERT_CE_LOGIT 1    /* pooler tanh + Linear(hidden, 1) logit        -> out_dev fp32 [batch] */
#define RMU_BERT_POOL_CLS 2    /* first token's state (+ L2 normalise)         -> out_dev fp32 [batch, out_stride] */
#define RMU_BERT_TOKENS 3      /* final hidden state of every real token (sentence-transformers output_value="token_embeddings"):
                                * packed rows, sequence b at rows [sum(len[<b]), +len[b]), len = min(lens, max_len)
                                *                                              -> out_dev fp32 [sum len, out_stride] */
#define RMU_BERT_NO_NORMALIZE 0x100 /* OR-ed into POOL_MEAN / POOL_CLS: the checkpoint has no Normalize module */
/* ids/type_ids: device int32 [batch, max_len] (row padded), lens: device int32 [batch], clipped to [0, max_len].  A sequence of
 * length 0 yields no TOKENS rows, a zero vector in POOL_MEAN / POOL_CLS (sentence-transformers' clamped mean of nothing) and the
 * head applied to a zero hidden state in CE_LOGIT; the other sequences get what they get without it (bit for bit when both
 * shapes take the same kernels, see below).
 * Rounding and batch shape: activations are bf16, and which kernels serve a call depends on batch * max_len (<= 2560 tokens with
 * max_len <= 256: the small-batch GEMMs; <= 16384: the GEMM pair; above: the fused FFN kernel) -- a sequence's result is bit-identical across
 * calls that take the same kernels and equal up to bf16 rounding noise (|d| < 2e-3 on unit vectors, cosine > 0.9999)
 * otherwise: a query embedded alone reproduces the vector its text got at indexing time to that noise, not bit for bit.
 * A GENERAL model has ONE set of kernels for every call size: a sequence's result is bit-identical whatever else is in the call.  Its
 * workspace is that of one group of whole sequences of at most 16384 packed tokens (a call is walked group by group), whatever the call size.
 * out_stride >= hidden.
 * hip_stream != 0: the forward is left in flight on that stream (inputs and out_dev must stay valid until it has run); the model's next
 * call on any OTHER stream -- stream 0 and the host-path entry points included -- is ordered behind it on the device (one workspace per
 * model), so a caller may queue the next block's forward while this one runs. */
int rmu_bert_encode(rmu_bert_t* m, const int32_t* ids, const int32_t* type_ids, const int32_t* lens,
                    int batch, int max_len, int mode, float* out_dev, int64_t out_stride,
                    uint64_t hip_stream);

/* The same forward for a HANDFUL of tokens (batch * max_len <= 4096 and <= 256 result rows: embed_query, the <= 14 (query, passage)
 * pairs of one rerank call) from HOST buffers to a HOST result: the interactive per-request pattern of the reference (one query per
 * /chat call, RAGHelper.py:497-499; ScoredCrossEncoderReranker.py:42).  The library replays one captured hipGraph per input shape
 * (H2D, ~45 launches, D2H: one graph launch, one synchronisation) and keeps the 64 most recently used shapes: callers should bucket
 * batch and max_len (a padded sequence has lens = 0 and costs nothing).
 * ids / type_ids (may be NULL) [batch, max_len], lens [batch]: host int32; out_host as out_dev above, on the host.
 * Tuned geometry only (a general model: RMU_E_INVALID, use rmu_bert_encode). */
int rmu_bert_encode_host(rmu_bert_t* m, const int32_t* ids, const int32_t* type_ids, const int32_t* lens,
                         int batch, int max_len, int mode, float* out_host, int64_t out_stride);

/* The reference's per-request retrieval as ONE call with ONE synchronisation (VectorStoreRetriever.invoke with search_type="mmr",
 * RAGHelper.py:497-499: embed_query -> dense top-fetch_k -> maximal_marginal_relevance): HOST token ids of `batch` queries in (as
 * rmu_bert_encode_host; mode = RMU_BERT_POOL_MEAN | RMU_BERT_POOL_CLS [| RMU_BERT_NO_NORMALIZE]), HOST out_rows [batch, k] int64 (row ids
 * + row_base in pick order, -1 past the number of candidates) and out_scores [batch, k] fp32 (the search score of each pick; may be
 * NULL) out.  The pooled query vectors stay on the device between the forward and the search (out_vecs, if not NULL, receives
 * them: [batch, 384] fp32).  lambda_mult < 0: no selection -- the top-k in score order (k <= fetch_k), i.e. rmu_index_search.
 * fetch_k <= 64, k <= fetch_k; the index must hold 384-d rows.  Results equal rmu_bert_encode_host + rmu_index_search_mmr.
 * Tuned geometry only (a general model: RMU_E_INVALID, use rmu_bert_encode + rmu_index_search_mmr). */
int rmu_bert_search_mmr(rmu_bert_t* m, rmu_index_t* idx, const int32_t* ids, const int32_t* type_ids, const int32_t* lens, int batch,
                        int max_len, int mode, int fetch_k, int k, double lambda_mult, int64_t row_base, int64_t* out_rows,
                        float* out_scores, float* out_vecs);

/* ---- WordPiece tokenizer (host C++; the step in front of both encoder forwards) --------------------
 * Restates transformers' BertTokenizer (BasicTokenizer + WordPiece) as used by sentence-transformers `tokenize`
 * (HuggingFaceEmbeddings.embed_documents, RAGHelper.py:423-434) and CrossEncoder pair tokenisation
 * (HuggingFaceCrossEncoder.score, RAGHelper.py:483-486).  vocab_path: one token per line (vocab.txt). */
typedef struct rmu_tok rmu_tok_t;
int rmu_tok_create(rmu_tok_t** out, const char* vocab_path, int do_lower_case);
int rmu_tok_free(rmu_tok_t* tk);
int rmu_tok_vocab_size(rmu_tok_t* tk);
/* n UTF-8 strings (texts_b may be NULL, or hold NULL entries, for single sentences).  Host outputs: ids/type_ids
 * [n, max_len] int32 ([CLS] a [SEP] (b [SEP]), [PAD]-filled; type_ids may be NULL), lens [n].  Single sequences keep
 * their first max_len-2 tokens; pairs use "longest_first" truncation. */
int rmu_tok_encode(rmu_tok_t* tk, const char* const* texts_a, const char* const* texts_b, int n, int max_len,
                   int32_t* ids, int32_t* type_ids, int32_t* lens);
/* The same over NUL-separated blobs: blob_a holds n strings back to back, each terminated by '\0' (bytes_a = total size including
 * the terminators); blob_b likewise or NULL.  One host buffer per call instead of n pointers: what a Python caller builds with a
 * single join + encode.  RMU_E_INVALID when a blob does not hold exactly n terminated strings. */
int rmu_tok_encode_blob(rmu_tok_t* tk, const char* blob_a, int64_t bytes_a, const char* blob_b, int64_t bytes_b, int n, int max_len,
                        int32_t* ids, int32_t* type_ids, int32_t* lens);

/* ---- BM25 retriever: inverted index in HBM, fused score + top-k (bm25.hip) -------------------------------------------
 * Serves: the sparse member of the reference's ensemble, BM25Retriever.from_texts(...) under EnsembleRetriever([sparse, dense],
 * weights=[0.5, 0.5]) (RAGHelper.py:436-443, :492-505; rebuilt after every upload, :529-531).  Okapi BM25 as rank_bm25.BM25Okapi computes it:
 *   tokens = Python's str.split() (whitespace = str.isspace(); case-sensitive, nothing stripped; an empty document has length 0);
 *   idf[t] = ln(N - df + 0.5) - ln(df + 0.5), every idf < 0 replaced by epsilon * mean(idf over the vocabulary, before replacement);
 *   score  = sum over the query's tokens in order (duplicates count each time, unknown tokens add 0) of
 *            idf[t] * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl)).
 * Every document is a candidate, zero and negative scores included.  Order: score descending, then LOWER document id -- rank_bm25's
 * argsort()[::-1] puts the higher id first among equal scores and is not stable, so equal-scoring documents may come back in another order.
 * Document ids are int64 numbers in insertion order.  The master postings live on the host (add_texts, stat and df never touch the GPU);
 * the first search packs them and uploads one image.  The first search after a later add packs and uploads only the added documents'
 * postings and splices them into the image on the device (host work O(vocabulary + new postings) + the O(N) doc_norm pass; the old postings
 * never cross the bus again) -- unless RMU_BM25_OPT_REPACK_ON_ADD is 1, or the image was not there: then it packs the whole image again.
 *
 * Live documents.  A document is LIVE until rmu_bm25_remove_docs removes it; a removed document keeps its id until rmu_bm25_compact, and no id is
 * reused before that.  Every search after a removal returns what rank_bm25.BM25Okapi built over the live documents in id order would return,
 * with ids mapped back: N is the number of live documents; df[t] counts the live documents that contain t; the vocabulary is the set of terms
 * with df > 0 (the mean idf of the epsilon replacement runs over those only, and a query token whose df has dropped to 0 contributes nothing,
 * like an unknown one); avgdl is the live token total over the live count.  Removed documents are never candidates, not even with score 0;
 * slots beyond the live count hold (-inf, -1); ties stay (score, then lower id).  An index whose documents are all removed answers like an
 * empty one and does no device work.  Not provided: the ParadeDB retriever. */
typedef struct rmu_bm25 rmu_bm25_t;
int rmu_bm25_create(rmu_bm25_t** out, double k1, double b, double epsilon);   /* rank_bm25's defaults: 1.5, 0.75, 0.25 */
int rmu_bm25_free(rmu_bm25_t* h);
/* Append n documents: blob holds n UTF-8 strings back to back, each terminated by '\0' (bytes = total size including the terminators, the
 * convention of rmu_tok_encode_blob).  *first_doc (may be NULL) = id of the first one.  Host only. */
int rmu_bm25_add_texts(rmu_bm25_t* h, const char* blob, int64_t bytes, int64_t n, int64_t* first_doc);
#define RMU_BM25_STAT_DOCS 1    /* ids handed out, removed documents included: what first_doc continues from */
#define RMU_BM25_STAT_VOCAB 2   /* distinct terms of the live documents */
#define RMU_BM25_STAT_NNZ 3     /* postings = (term, live document) pairs */
#define RMU_BM25_STAT_AVGDL 4   /* mean tokens per live document (0 when there is none) */
#define RMU_BM25_STAT_LIVE_DOCS 5 /* live documents */
/* Counters of the device image, all 0 until the first search (host-only reads like the others): */
#define RMU_BM25_STAT_IMAGE_PACKS 16        /* full packs: every master posting packed on the host and uploaded */
#define RMU_BM25_STAT_IMAGE_SPLICES 17      /* splices: only the added documents' postings packed and uploaded, the image re-laid on the device */
#define RMU_BM25_STAT_IMAGE_UPLOAD_BYTES 18 /* host-to-device bytes of postings and posting pointers so far, both paths (not: doc_norm, bitmap, descriptors) */
int rmu_bm25_stat(rmu_bm25_t* h, int what, double* out);
/* Live documents that contain the term (0 for an unknown one).  Host only. */
int rmu_bm25_df(rmu_bm25_t* h, const char* term_utf8, int64_t* df);
/* Testing switches: results are identical, bit for bit, for every value (the tests force many tiles, many workgroups and range boundaries on
 * small corpora through them).  0 = default. */
#define RMU_BM25_OPT_TILE_DOCS 1  /* documents per LDS tile: a power of two in [64, 8192] */
#define RMU_BM25_OPT_MAX_WGS 2    /* workgroups per query (= part lists of the final merge), at most 1024 */
#define RMU_BM25_OPT_REPACK_ON_REMOVE 4 /* 0 or 1.  1: a removal marks the image dirty (the next search repacks it without the removed documents'
                                         * postings) instead of stale (the next search refreshes weights, doc_norm and the liveness bitmap only) */
#define RMU_BM25_OPT_REPACK_ON_ADD 8    /* 0 or 1.  1: an add marks the image dirty (the next search packs and uploads every posting again)
                                         * instead of grown (the next search uploads the added postings and splices them in on the device) */
int rmu_bm25_set_option(rmu_bm25_t* h, int option, int64_t value);
/* Top-k of nq queries (a NUL-separated blob like add_texts'; at most 1024 tokens per query, 1 <= nq <= 65535, 1 <= k <= RMU_MAX_K; otherwise
 * RMU_E_INVALID before anything is enqueued).  HOST outputs out_scores [nq, k] fp32 and out_docs [nq, k] int64 (+ doc_base), best first;
 * slots beyond N hold (-inf, -1).  hip_stream: 0 = an internal per-thread stream, otherwise the work is ordered on that stream; either way the
 * results are host arrays, so the stream has been drained when the call returns. */
int rmu_bm25_search(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, float* out_scores,
                    int64_t* out_docs, uint64_t hip_stream);
/* Remove documents.  Host only, never touches the GPU.  An id outside [0, DOCS) gives RMU_E_INVALID and changes nothing; an id that is already
 * removed, or given twice, counts once or not at all; *n_removed (may be NULL) = the documents that were live.  Recounts df in one pass over
 * the master postings -- O(postings) per CALL, so batch the ids -- and marks the device image stale: the first search afterwards recomputes the
 * weights and doc_norm from the live statistics and uploads them with a liveness bitmap (4 bytes + 1 bit per document); the postings image is
 * not repacked, and the postings of removed documents stay in it until the next repack (a compact; an add splices and keeps them, unless
 * RMU_BM25_OPT_REPACK_ON_ADD is set).  Results are the same, bit for bit, on either path. */
int rmu_bm25_remove_docs(rmu_bm25_t* h, const int64_t* docs, int64_t n, int64_t* n_removed);
/* rmu_bm25_search over a subset: the candidates are the LIVE documents of docs[0, n_sub), a HOST list of strictly ascending document ids
 * (checked before anything is enqueued: not ascending, or outside [0, DOCS), gives RMU_E_INVALID); one list serves all queries.  The statistics
 * stay the whole live corpus's, as a Milvus or ParadeDB filter leaves them: every returned score has the bits rmu_bm25_search returns for that
 * document.  n_sub == 0, or fewer than k live documents in the list, fills the rest with (-inf, -1).  Everything else is rmu_bm25_search's
 * contract.  The call ships a bitmap of N / 8 bytes with its descriptors; its time follows the postings of the query's terms, NOT the length
 * of the list (every posting of a query term is still scored; only the selection is restricted). */
int rmu_bm25_search_subset(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base, const int64_t* docs,
                           int64_t n_sub, float* out_scores, int64_t* out_docs, uint64_t hip_stream);
/* rmu_bm25_search_subset with ONE LIST PER GROUP OF QUERIES, in one call (rmu_index_search_groups' contract, transposed to documents): many
 * concurrent requests, each filtered to its own upload, share one launch.  docs = n_lists HOST lists laid end to end, list g =
 * docs[list_ptr[g] .. list_ptr[g + 1]) (list_ptr[0] = 0, list_ptr non-decreasing), each strictly ascending ids in [0, DOCS); lists may overlap,
 * repeat each other, be empty or go unused.  q_list[i] in [0, n_lists) = the list of query i; it must be NON-DECREASING (the caller reorders
 * its queries, the library does not).
 * Result of query i: exactly what rmu_bm25_search_subset(h, query i, 1, k, doc_base, list q_list[i]) returns -- the same order (score, then
 * lower id), the same (-inf, -1) padding, no removed document, every score bit for bit.  The bits cannot move: a document's score is the fp32
 * sum over the query's terms in order with one posting per term, so it depends neither on the tile nor on the range a workgroup covers; the
 * statistics (N, df, idf, avgdl) stay the whole live corpus's.
 * Limits (RMU_E_INVALID with a message, before anything is enqueued; the lists are checked under the handle's shared lock, and again after the
 * lock was given up for an image rebuild): those of rmu_bm25_search -- 1 <= nq <= 65535, at most 1024 tokens per query, 1 <= k <= RMU_MAX_K --
 * and n_lists >= 1.  No device work at all when nothing is live or no used list holds a live document.  Outputs are HOST arrays; the stream
 * has been drained when the call returns.
 * Work: unlike the subset call, the time FOLLOWS THE LISTS.  The host keeps, per used list, only the tiles that hold a live candidate; runs
 * of kept tiles become the document ranges of a work table, cut so that a long list still spreads over the CUs and joined across empty tiles
 * so that no query has more than RMU_BM25_OPT_MAX_WGS parts; one workgroup scores one range for one query.  Only the mask words of kept
 * ranges (allow AND live; the queries of a list share them) are built and uploaded, never n_lists x N / 8 bytes.  One scoring launch and one
 * merge however many lists there are.  RMU_BM25_OPT_TILE_DOCS and RMU_BM25_OPT_MAX_WGS are honoured.
 * Serves: the sparse member of the ensemble (RAGHelper.py:497-503) for a BATCH of requests whose filters differ -- every user asking about
 * their own upload -- which the reference answers one retriever call per request. */
int rmu_bm25_search_groups(rmu_bm25_t* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t doc_base,
                           const int64_t* docs, const int64_t* list_ptr, int n_lists, const int32_t* q_list,
                           float* out_scores, int64_t* out_docs, uint64_t hip_stream);
/* Reclaim removed documents (the contract of rmu_index_compact): live documents keep their order and become 0 .. n_live-1.  old_to_new
 * [map_len] receives the new id of every old one, -1 for removed ids and for the entries [DOCS, map_len); map_len < DOCS gives RMU_E_INVALID
 * and changes nothing.  *n_after (may be NULL) = documents afterwards.  With no removed document nothing changes and the image stays clean.
 * Host only: the next search repacks the whole image (adds after that are spliced in again).  Term ids stay; a term left without postings is out of the statistics.  Results afterwards
 * equal those before with ids mapped, bit for bit. */
int rmu_bm25_compact(rmu_bm25_t* h, int64_t* old_to_new, int64_t map_len, int64_t* n_after);
/* One flat little-endian file: "RMUBM25\0", u32 version (1), u32 0 | f64 k1, b, epsilon | u64 N, V, nnz | u32 dl[N] | u8 liveness[N] | the V
 * terms in term-id order, each u32 length + bytes | u64 posting offsets[V + 1] | u32 posting documents[nnz] | u32 posting tfs[nnz].  Removed
 * documents survive as removed (as in rmu_index_save); options do not.  Host only.  load checks every size against the file's length before
 * it allocates, and that each term's postings ascend inside [0, N), tfs are >= 1 and dl equals the tf sums: a short, long or inconsistent
 * file gives RMU_E_INVALID with a message.  A loaded index answers every search with the bits the saved one gave. */
int rmu_bm25_save(rmu_bm25_t* h, const char* path);
int rmu_bm25_load(rmu_bm25_t** out, const char* path);

/* ---- hybrid retrieval: reciprocal-rank fusion on the device, and the ensemble's whole retrieval step as one call (rrf_fuse.hip) ----------
 * Serves: EnsembleRetriever([bm25, dense_mmr], weights=[0.5, 0.5]).invoke, the only retrieval call of the reference's chains
 * (RAGHelper.py:497-503, RAGHelper_local.py:251-259): langchain's weighted_reciprocal_rank with c = 60, documents identified by page_content.
 *
 * rmu_rrf_fuse: weighted reciprocal-rank fusion of `lists` ranked key lists per query.  keys [lists, nq, depth] int64, best first; a key is >= 0,
 * -1 = absent (anywhere in a list).  Per query, with the entries taken in CHAIN order (list 0 first, positions ascending):
 *   rank   = 1 + the present entries in front of the entry in its own list (an absent slot consumes no rank);
 *   score  = the fp64 sum, in chain order from 0.0, of weights[l] / (rank + c) over every entry holding the key (duplicates inside a list count);
 *   output = the distinct keys, score descending, equal scores in order of their first entries -- Python's stable sort over first-seen order, so
 *            with equal weights rank r of list 0 comes before rank r of list 1.
 * The quotients are computed on the host and only added on the device, in Python's order: out_scores has the bits of
 * ragmeup_amd.ensemble.weighted_reciprocal_rank's sums.  out_scores [nq, k_out] fp64, out_keys [nq, k_out] int64, out_src [nq, k_out] int32 =
 * list * depth + position of the key's first entry; slots beyond the distinct keys hold (-inf, -1, -1).
 * weights [lists]: HOST fp64, finite and >= 0; c >= 0; 1 <= lists <= RMU_RRF_MAX_LISTS, 1 <= depth <= RMU_MAX_K, 1 <= k_out <= lists * depth,
 * 1 <= nq; anything else is RMU_E_INVALID before any HIP call.  flags: RMU_F_Q_DEVICE (keys is a device address), RMU_F_OUT_DEVICE (the three
 * outputs are).  hip_stream as rmu_topk_merge: drained on return unless a caller stream is given with device keys AND device outputs. */
#define RMU_RRF_MAX_LISTS 4
int rmu_rrf_fuse(const int64_t* keys, int lists, int64_t nq, int depth, const double* weights, int c, int k_out,
                 unsigned flags, double* out_scores, int64_t* out_keys, int32_t* out_src, uint64_t hip_stream);

/* The two members of the ensemble behind one handle.  The members are BORROWED: never freed here, and they must outlive the handle.  Either
 * may be NULL (not both): an absent member contributes an empty list and its key table must stay empty. */
typedef struct rmu_hybrid rmu_hybrid_t;
int rmu_hybrid_create(rmu_hybrid_t** out, rmu_bm25_t* sparse, rmu_index_t* dense);
int rmu_hybrid_free(rmu_hybrid_t* h);
/* The identity of the members' records: keys[i] = key of document id / row id first + i of `member` (0 = sparse, 1 = dense); two records are
 * the same document iff their keys are equal (the host numbers the classes of page_content).  Writes [first, first + n) of the member's table
 * from a HOST array; first <= the table's current length, which becomes first + n: first = 0 replaces the table, first = length appends, n = 0
 * truncates.  Every key >= 0.  Host only (the device copy follows at the next search); RMU_E_INVALID changes nothing. */
int rmu_hybrid_set_keys(rmu_hybrid_t* h, int member, int64_t first, const int64_t* keys, int64_t n);
/* The retrieval step in ONE call with ONE synchronisation.  HOST q [nq, dim of the dense member] fp32 and the NUL-separated query blob of
 * rmu_bm25_search (the same nq queries as text).  On one stream (hip_stream, or the calling thread's own) it enqueues rmu_bm25_search's work for
 * k_sparse, rmu_index_search_mmr's for (fetch_k, k_dense, lambda_mult; lambda_mult < 0: no selection, the top-k_dense in score order, as in
 * rmu_bert_search_mmr), the fusion of the two lists read through the key tables -- the sparse list is list 0 -- and one copy of the results;
 * then it drains the stream.  The two lists inside the call are, bit for bit, what those two calls return on their own, and the fusion is
 * rmu_rrf_fuse's over their keys.
 * HOST outputs, [nq, k_out] each: out_scores fp64; out_ids int64 and out_member int32 name each fused hit by the first entry that holds its key:
 * the member (0 / 1) and that member's own id (document id / row id).  Slots beyond the distinct keys hold (-inf, -1, -1).
 * weights [2] (sparse, dense) and c as rmu_rrf_fuse; 1 <= k_out <= k_sparse + k_dense.
 * Checked before anything is enqueued, the members' records under their shared locks: every limit of rmu_bm25_search and rmu_index_search_mmr,
 * and that each table is as long as its member (BM25 DOCS / index rows) -- otherwise RMU_E_INVALID with a message that contains "out of step":
 * the caller refreshes the table and repeats the call.  Ids the tables do not cover can therefore not occur.  A member with nothing live
 * contributes an empty list (BM25: no device work). */
int rmu_hybrid_search(rmu_hybrid_t* h, const float* q, int64_t nq, const char* query_blob, int64_t bytes,
                      int k_sparse, int fetch_k, int k_dense, double lambda_mult, const double* weights /* [2]: sparse, dense */, int c,
                      int k_out, double* out_scores, int64_t* out_ids, int32_t* out_member, uint64_t hip_stream);
/* The same call behind the encoder forward (the pattern of rmu_bert_search_mmr): HOST token ids of `batch` queries in (as rmu_bert_encode_host;
 * a pooling mode), their texts in query_blob; the pooled vectors stay on the device, everything runs on the encoder's stream, one
 * synchronisation.  The dense member must hold 384-d rows.  Results equal rmu_bert_search_mmr's rows and rmu_bm25_search's documents fused. */
int rmu_bert_search_hybrid(rmu_bert_t* m, rmu_hybrid_t* h, const int32_t* ids, const int32_t* type_ids, const int32_t* lens, int batch,
                           int max_len, int mode, const char* query_blob, int64_t bytes, int k_sparse, int fetch_k, int k_dense,
                           double lambda_mult, const double* weights, int c, int k_out, double* out_scores, int64_t* out_ids,
                           int32_t* out_member);

/* ---- semantic chunker: the cosine distance of adjacent rows (semantic.hip) ------------------------------------------------------------
 * Serves: SemanticChunker(self.embeddings, breakpoint_threshold_type=..., ...) (RAGHelper.py:329-349): the splitter embeds one window per
 * sentence and thresholds ONE number per adjacent pair of windows.  ragmeup_amd/chunker.py is the host half (sentences, windows, thresholds).
 *
 * out[i] = 1 - sim(x[i], x[i+1]), i in [0, n-1):  sim = dot / (sqrt(|a|^2) * sqrt(|b|^2)); dot, |a|^2, |b|^2 are fp64 sums of the
 * (exact) fp64 products of the fp32 inputs; a quotient that is NaN or +-Inf (a zero row, a NaN / Inf element) counts as sim = 0, so out = 1.0.
 * The order of the additions is fixed by the element index alone (element e belongs to lane (e >> 2) & 63, a lane adds its elements ascending,
 * the lanes are folded by an xor butterfly over 32 .. 1): out[i] has the same bits whatever n, wherever the pair sits in the call, whether or
 * not the base and stride allow 16-byte loads, and on any stream.
 * x [n, stride] fp32, of which columns dim .. stride-1 are never read: a device address with RMU_F_Q_DEVICE, else a host array (uploaded
 * asynchronously).  out [n-1] fp64: a device address with RMU_F_OUT_DEVICE, else a host array.  n == 1 writes nothing and launches nothing.
 * 1 <= dim <= RMU_MAX_DIM_WIDE, stride >= dim, n >= 1; a NULL pointer, any other flag, any other value: RMU_E_INVALID before any HIP call.
 * hip_stream as rmu_topk_merge: drained on return unless a caller stream is given with a device x AND a device out. */
int rmu_adjacent_cosine(const float* x, int64_t n, int dim, int64_t stride, unsigned flags, double* out, uint64_t hip_stream);

/* ---- similarity provenance: the share of an answer each retrieved document accounts for (provenance.hip) ------------------------------
 * Serves: DocumentSimilarityAttribution.compute_similarity(query, context, answer) (provenance.py:164-202, provenance_method=similarity;
 * RAGHelper_local.py:294-295 calls it once per /chat request).  ragmeup_amd/provenance.py is the host half (texts, the group table, the class).
 *
 * A group is one request: an answer row, an optional query row and n_docs consecutive document rows of x.  For document i of a group
 *   sim_a = sim(doc_i, answer), sim_q = sim(doc_i, query);  s_i = sim_a without a query, else (sim_a + sim_q) / 2;
 *   T = s_0 + s_1 + ..., accumulated from +0.0 in document order;  out_scores = s_i / T (a true division) if T > 0, else s_i.
 * sim = dot / (sqrt(|a|^2) * sqrt(|b|^2)); dot, |a|^2, |b|^2 are fp64 sums of the (exact) fp64 products of the fp32 inputs; a quotient that is
 * NaN or +-Inf (a zero row, a NaN / Inf element) counts as sim = 0.  The order of the additions is fixed by the element index alone (element e
 * belongs to lane (e >> 2) & 63, a lane adds its elements ascending with fma from +0.0, the lanes are folded by an xor butterfly over 32 .. 1):
 * a group's outputs have the same bits wherever the group and its rows sit in the call, whether or not the base and stride allow 16-byte loads,
 * at every width and on any stream.
 * x [n, stride] fp32, of which columns dim .. stride-1 are never read: a device address with RMU_F_Q_DEVICE, else a host array (uploaded
 * asynchronously).  groups: ALWAYS a host array, [n_groups, 4] int32 = answer_row, query_row (-1: none), first_doc_row, n_docs.  Rows may be
 * shared between groups and may coincide with an anchor.  The outputs are packed in group order -- out_scores [sum n_docs] fp64, out_sims
 * [sum n_docs, 2] fp64 = the unnormalised (sim_a, sim_q; sim_q = 0.0 without a query), or NULL -- device addresses with RMU_F_OUT_DEVICE,
 * else host arrays.  n_groups == 0 and groups with n_docs == 0 write nothing (no document at all: nothing is launched).
 * 1 <= dim <= RMU_MAX_DIM_WIDE, stride >= dim, n >= 1, n_groups >= 0; every row in [0, n), n_docs >= 0, first_doc_row + n_docs <= n, the sum
 * of n_docs fits in an int32; a NULL pointer (out_sims aside), any other flag, any other value: RMU_E_INVALID before any HIP call.
 * hip_stream: the stream the work is enqueued on (0: the calling thread's own).  The call ALWAYS drains it before it returns: the table
 * travels through the thread's pinned workspace, so nothing may stay in flight. */
int rmu_attribution(const float* x, int64_t n, int dim, int64_t stride, const int32_t* groups, int n_groups, unsigned flags,
                    double* out_scores, double* out_sims, uint64_t hip_stream);
/* The same behind the encoder forward (the pattern of rmu_bert_search_mmr): HOST token ids of the answers, queries and contexts of one or more
 * requests in (as rmu_bert_encode_host, with its shape limits; a pooling mode); the group table names rows of that batch (n = batch, dim = 384).
 * The pooled vectors stay on the device, the kernel is enqueued behind the graph replay on the encoder's stream, one synchronisation.  HOST
 * outputs as above; out_vecs, if not NULL, receives the pooled vectors [batch, 384] fp32.  The table is checked before anything is enqueued.
 * Results equal rmu_bert_encode_host followed by rmu_attribution on its output. */
int rmu_bert_attribute(rmu_bert_t* m, const int32_t* ids, const int32_t* type_ids, const int32_t* lens, int batch, int max_len, int mode,
                       const int32_t* groups, int n_groups, double* out_scores, double* out_sims, float* out_vecs);

/* ---- rerank by key: passage tokens in HBM, pairs assembled and the top-n selected on the device (rerank.hip) ---------------------------
 * Serves: ContextualCompressionRetriever(base_compressor=ScoredCrossEncoderReranker(model, top_n), base_retriever=ensemble).invoke
 * (RAGHelper.py:476-490, RAGHelper_local.py:157-159), and the same compressor run once more per /chat request with the answer as the query
 * (provenance.py:100-108): score every (query, page_content) pair, Python's stable sorted(..., reverse=True), keep top_n
 * (ScoredCrossEncoderReranker.py:42-45).  ragmeup_amd/rerank.py is the host half (the text -> key dictionary, the retriever).
 *
 * The table holds one entry per KEY (a distinct passage text; the host numbers them): the passage's WordPiece ids WITHOUT special tokens.  An
 * entry keeps the first max_len - 3 of its tokens -- the most a pair can ever hold of its second text -- and remembers how long it was: the
 * truncation rule below asks which side was longer.  Host side and device image; create / free / size / set never touch a GPU (the image
 * follows at the next rerank call: the tail only, re-allocated when it does not fit).  8 <= max_len <= 512, special ids >= 0. */
typedef struct rmu_passages rmu_passages_t;
#define RMU_RERANK_MAX_M 256      /* candidates per query */
int rmu_passages_create(rmu_passages_t** out, int cls_id, int sep_id, int pad_id, int max_len);
int rmu_passages_free(rmu_passages_t* p);
int rmu_passages_size(rmu_passages_t* p, int64_t* n_entries, int64_t* n_tokens);      /* either may be NULL; n_tokens: the tokens KEPT */
/* entries [first, first + n) := tokens[offsets[i] .. offsets[i + 1]), i in [0, n); the table ends at first + n afterwards: first = size appends,
 * first < size truncates first, n = 0 only truncates; first > size is RMU_E_INVALID with a message that contains "out of step".  HOST arrays;
 * offsets [n + 1] ascending from 0; a token id < 0 is RMU_E_INVALID.  RMU_E_INVALID changes nothing. */
int rmu_passages_set(rmu_passages_t* p, int64_t first, const int32_t* tokens, const int64_t* offsets, int64_t n);
/* The assembled pairs themselves: row q * m + j = [CLS] query q [SEP] passage keys[q, j] [SEP] [PAD]..., token types 0 0 0 1 1 0..., its length;
 * what rmu_tok_encode writes for the two texts at this max_len, id for id.  (n1, n2) tokens of the two sides follow "longest_first": nothing
 * is cut when both fit max_len - 3; only the longer side when that suffices; else both go to half the budget, the odd token to the longer
 * side, to the passage on equal lengths.  A key of -1 (rmu_hybrid_search's padding) gives a row of [PAD] with length 0.
 * HOST arrays throughout.  q_tokens [nq, q_stride]: the queries' WordPiece ids without special tokens, q_lens [nq]: their lengths -- which may
 * exceed q_stride as long as the row holds the head the pair can use, min(length, max_len - 3) tokens; keys [nq, m] in [-1, size);
 * outputs ids / type_ids [nq * m, max_len], lens [nq * m].  1 <= m <= RMU_RERANK_MAX_M, 1 <= nq, nq * m <= 65535, 8 <= max_len <= the
 * table's; anything else is RMU_E_INVALID before anything is enqueued.  Runs on the calling thread's stream, drained on return. */
int rmu_passages_pairs(rmu_passages_t* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride,
                       const int64_t* keys /* [nq, m] */, int m, int max_len, int32_t* ids, int32_t* type_ids, int32_t* lens);
/* The stable top-n of m candidates per query: logits [nq, m] fp32, keys [nq, m] int64 (< 0: absent, never output).  out_pos [nq, top_n] int32
 * = positions in the candidate list, out_scores [nq, top_n] fp32 = their logits, bit for bit, in the order of Python's
 * sorted(zip(docs, scores), key=itemgetter(1), reverse=True): logit descending, equal logits (+0.0 == -0.0) by position; a NaN ranks behind
 * every number, NaNs among themselves by position.  Slots beyond the present candidates hold (-1, -inf).
 * 1 <= m <= RMU_RERANK_MAX_M, 1 <= top_n <= 65535, 1 <= nq <= 65535.  flags: RMU_F_Q_DEVICE (logits and keys are device addresses),
 * RMU_F_OUT_DEVICE (the two outputs are).  hip_stream as rmu_topk_merge: drained on return unless a caller stream is given with device inputs
 * AND device outputs. */
int rmu_rerank_select(const float* logits, const int64_t* keys, int64_t nq, int m, int top_n, unsigned flags,
                      int32_t* out_pos, float* out_scores, uint64_t hip_stream);
/* The rerank step in ONE call with ONE synchronisation: HOST query tokens and keys in (as rmu_passages_pairs), HOST top-n out (as
 * rmu_rerank_select; out_logits [nq, m_cand], may be NULL, receives every pair's logit).  On the encoder's stream: the copy of queries and keys,
 * the table's pending tail, the pair assembly, the RMU_BERT_CE_LOGIT forward over batch_pad rows of max_len (rows past nq * m_cand have length
 * 0), the selection, the copies back.  (batch_pad, max_len) is the shape the forward runs at -- the caller's bucketing, as for
 * rmu_bert_encode_host: up to batch_pad * max_len = 4096 the forward is that call's captured graph in a form that reads its inputs from the
 * device, beyond it rmu_bert_encode's launches.  out_logits has the bits of rmu_bert_encode_host (rmu_bert_encode beyond 4096 tokens) over
 * rmu_passages_pairs' arrays padded to the same shape.  The model needs a classification head; nq * m_cand <= batch_pad <= 65535,
 * max_len <= the table's and the model's; every limit of the two calls above; otherwise RMU_E_INVALID before anything is enqueued. */
int rmu_bert_rerank(rmu_bert_t* m, rmu_passages_t* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride,
                    const int64_t* keys, int m_cand, int batch_pad, int max_len, int top_n,
                    int32_t* out_pos, float* out_scores, float* out_logits /* [nq, m_cand], may be NULL */);

/* ---- metadata columns in HBM: the row lists of a filtered search built on the device (columns.hip) -------------------------------------
 * Serves: the step IN FRONT of rmu_index_search_subset / rmu_index_search_groups -- which rows does expr='source == "a.pdf"' name
 * (RAGHelper.py:497-499 with search_kwargs) -- which a host otherwise answers by walking its records after every upload or delete
 * (server.py:150-183, 353-385; RAGHelper.py:518-538) and ships as 8 bytes per selected row on every call.
 *
 * The columns hold one int32 code per row and field, 1..8 fields.  The HOST numbers the values of each field; the library sees only codes
 * >= 0.  A host master copy lives behind the handle: create, append, size, compact, set_option and free never touch the GPU.  The device
 * image is field-major (one contiguous int32 array per field) and follows at the next selection: only the tail is uploaded, and the image is
 * re-allocated only when the rows no longer fit.  Rows are the index's rows: append where the index appends, compact with the map
 * rmu_index_compact returned.  A removed (tombstoned) row keeps its codes: selections may name it, the scan never returns it.
 * Thread-safe: selections on one handle run concurrently (shared lock, scratch belongs to the calling thread); append, compact and
 * set_option are exclusive. */
typedef struct rmu_columns rmu_columns_t;
int rmu_columns_create(rmu_columns_t** out, int n_fields, int64_t capacity_hint);
int rmu_columns_free(rmu_columns_t* c);
int rmu_columns_size(rmu_columns_t* c, int64_t* n_rows, int* n_fields);      /* either output may be NULL */
/* codes [n, n_fields] row-major HOST int32, every code >= 0; *first_row (may be NULL) = row of codes[0].  RMU_E_INVALID changes nothing. */
int rmu_columns_append(rmu_columns_t* c, const int32_t* codes, int64_t n, int64_t* first_row);
/* Apply the old_to_new map rmu_index_compact returned (map_len >= rows, otherwise RMU_E_INVALID and nothing changes; -1 = dropped; the kept
 * rows must map to 0, 1, 2, ... in order); *n_after (may be NULL) = rows afterwards. */
int rmu_columns_compact(rmu_columns_t* c, const int64_t* old_to_new, int64_t map_len, int64_t* n_after);
#define RMU_COLUMNS_OPT_TILE_ROWS 1   /* testing switch: rows per workgroup tile of the selection kernels, a power of two in [64, 16384]; 0 = default
                                       * (4096 = 256 lanes x 16 rows).  Small corpora cross tile boundaries, wave boundaries and the width of
                                       * the scan's block through it.  Results are identical for every value. */
int rmu_columns_set_option(rmu_columns_t* c, int option, int64_t value);

/* A SELECTION is a conjunction of 1..4 terms; a term is (field, accepted codes): the row's code in that field is one of them.  The accepted
 * codes of a term are strictly ascending (an empty set matches no row), and a selection carries at most 1024 codes in all.  The selections
 * of a call are passed flattened: terms [n_terms], codes [], sel_ptr [n_sel + 1] into terms (sel_ptr[0] = 0, sel_ptr[n_sel] = n_terms);
 * selection g = terms[sel_ptr[g] .. sel_ptr[g + 1]), term t accepts codes[codes_begin .. codes_end).  All three are HOST arrays, checked
 * before anything is enqueued: a field outside [0, n_fields), unsorted, repeated or negative codes, more than 4 terms, no term, more than
 * 1024 codes, or n_sel outside [1, 8192] gives RMU_E_INVALID with a message that names the selection. */
typedef struct rmu_col_term {
    int32_t field;
    int32_t codes_begin;
    int32_t codes_end;
} rmu_col_term;

/* The rows in [0, rows) whose codes satisfy selection g, ascending, the lists laid end to end: list g = out_rows[list_ptr[g] .. list_ptr[g + 1]).
 * list_ptr [n_sel + 1]: HOST, always written (the stream is drained).  out_rows: int64, HOST or (RMU_F_OUT_DEVICE, the only flag) DEVICE, room
 * for out_cap entries; NULL = count only.  out_cap < list_ptr[n_sel]: RMU_E_INVALID, list_ptr still holds the offsets, nothing else is written.
 * Work: one pass over the named columns per selection to count (one count per tile), an exclusive scan per selection and one over the
 * totals -- list_ptr is all the host reads, one synchronisation --, one pass to write; the lists come out ascending by construction. */
int rmu_columns_select(rmu_columns_t* c, const rmu_col_term* terms, int n_terms, const int32_t* codes, const int32_t* sel_ptr, int n_sel,
                       unsigned flags, int64_t* out_rows, int64_t out_cap, int64_t* list_ptr, uint64_t hip_stream);

/* Selection + rmu_index_search_groups in one call: query i is searched over the rows of selection q_sel[i] (HOST int32 [nq], NON-DECREASING,
 * as q_list there).  The lists never leave the device.  Result of query i: exactly -- bit for bit, order, padding -- what
 * rmu_index_search_subset returns for the HOST list of those rows.  Tombstoned rows never appear (the scan's own rule).
 * Selections that no query names are not evaluated; a selection without rows costs its queries no scan work (they get the (-inf | +inf, -1)
 * padding); when every named selection is empty no scan is launched.
 * The columns and the index must hold the same number of rows: otherwise RMU_E_INVALID, the message contains "out of step", nothing is
 * enqueued.  Limits and flags (RMU_F_Q_DEVICE, RMU_F_OUT_DEVICE, row_base, k, nq <= 8192, rows of at most RMU_MAX_DIM dimensions) are
 * rmu_index_search_groups', checked before anything is enqueued; the call always drains its stream. */
int rmu_index_search_where(rmu_index_t* idx, rmu_columns_t* c, const float* q, int64_t nq, int k, unsigned flags, int64_t row_base,
                           const rmu_col_term* terms, int n_terms, const int32_t* codes, const int32_t* sel_ptr, int n_sel,
                           const int32_t* q_sel, float* out_scores, int64_t* out_rows, uint64_t hip_stream);

/* GROUPED search: the best row of each of the k best groups (Milvus group_by_field; "one chunk per document").  `field` names one column
 * of `c`, whose codes are the groups; the columns must be in step with the index.  For each query, take all live rows in the order
 * rmu_index_search returns them -- score descending, then lower row id (RMU_METRIC_L2SQ: distance ascending, then lower row id) -- walk
 * that order and keep a row if and only if no kept row has the same code in `field`; the first k kept rows are the answer, in that order.
 * So every group is represented by its best row (the lowest id among bit-equal best scores) and the k best groups come out ordered by
 * their representatives.  Every returned score has exactly the bits rmu_index_search gives that row.  Tombstoned rows never appear and
 * never represent a group; a group whose rows are all removed is absent; with fewer than k live groups the remaining slots hold
 * (-inf | +inf for L2SQ, -1).  Exact: a selection that knows the groups (scan_distinct.hip), not an over-fetch -- one group may own
 * any number of the best rows.  An empty index, or one without a live row, gives all padding and launches no scan.
 * flags: RMU_F_Q_DEVICE, RMU_F_OUT_DEVICE; row_base is added to the returned ids; all three metrics; any nq >= 1 (more than 8192 queries
 * are sent in blocks).  RMU_E_INVALID with a message, before anything is enqueued: a null pointer, nq < 1, k outside
 * [1, RMU_MAX_K_DISTINCT], `field` outside [0, n_fields), an unknown flag, an index of rows wider than RMU_MAX_DIM (a wide index is not
 * served), columns and index holding different row counts (the message contains "out of step").  Lock order: the columns' lock, then the
 * index's; the call always drains its stream.  Not built: k > 32, a filter beside the grouping, wide rows, more than one row per group. */
#define RMU_MAX_K_DISTINCT 32
int rmu_index_search_distinct(rmu_index_t* idx, rmu_columns_t* c, int field, const float* q, int64_t nq, int k, unsigned flags,
                              int64_t row_base, float* out_scores, int64_t* out_rows, uint64_t hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RMU_H_ */
