// rmu_internal.h -- what the composite entry points of bert.hip (rmu_bert_search_mmr, rmu_bert_attribute, rmu_bert_search_hybrid,
// rmu_bert_rerank) call in the other units of librmu.so.  Internal symbols (trailing underscore): not in include/rmu.h, not in the Python
// binding's list.  bert.hip AND every defining unit include this header, so the compiler holds caller and definition to one prototype
// (extern "C" functions cannot be overloaded: a definition that drifts from its declaration here does not compile).
#pragma once
#include <stdint.h>
#include "../../include/rmu.h"

extern "C" {
// rmu_api.hip: rmu_index_search_mmr behind an encoder forward -- DEVICE queries on the encoder's stream; drains it
int rmu_index_search_mmr_dev_(rmu_index_t* idx, const float* q_dev, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t row_base,
                              int64_t* out_rows, float* out_scores, void* hip_stream);

// provenance.hip: the table against `n` encoder rows before the forward (no HIP call) ...
int rmu_attribution_check_(const char* who, int64_t n, int dim, const int32_t* groups, int n_groups, const double* out_scores, int64_t* total);
// ... and the kernel behind it: DEVICE rows on the encoder's stream, HOST results; drains the stream
int rmu_attribution_dev_(const char* who, const float* x_dev, int64_t n, int dim, int64_t stride, const int32_t* groups, int n_groups,
                         int64_t total, double* out_scores, double* out_sims, void* hip_stream);

// rrf_fuse.hip: the limits of rmu_hybrid_search alone, in front of the forward (*dense: the dense member); then the same call over DEVICE
// queries on the encoder's stream
int rmu_hybrid_check_(rmu_hybrid_t* h, rmu_index_t** dense, int64_t nq, const char* query_blob, int64_t bytes, int k_sparse, int fetch_k,
                      int k_dense, const double* weights, int c, int k_out, double* out_scores, int64_t* out_ids, int32_t* out_member);
int rmu_hybrid_search_dev_(rmu_hybrid_t* h, const float* q_dev, int64_t nq, const char* query_blob, int64_t bytes, int k_sparse, int fetch_k,
                           int k_dense, double lambda_mult, const double* weights, int c, int k_out, double* out_scores, int64_t* out_ids,
                           int32_t* out_member, void* hip_stream);

// rerank.hip: the steps of rmu_rerank on the encoder's stream, in front of and behind its forward.
// check: every limit of the call but the model's, the table's under its shared lock -- which, with `lock` (a
// std::shared_lock<std::shared_mutex>*) given, is handed back HELD (the caller releases it once it has drained the stream); no HIP call
int rmu_rerank_check_(rmu_passages_t* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride, const int64_t* keys,
                      int m, int batch_pad, int max_len, int top_n, const void* out_pos, const void* out_scores, void* lock);
// workspace: the thread's, for the shapes the encoder's own staging does not hold: ids | type ids | lens | logits of batch_pad rows
int rmu_rerank_workspace_(int batch_pad, int max_len, int32_t** d_in, float** d_logits);
// assemble: d_in = ids [batch_pad, max_len] | type ids | lens [batch_pad] (the encoder's staging layout)
int rmu_rerank_assemble_(rmu_passages_t* p, const int32_t* q_tokens, const int32_t* q_lens, int64_t nq, int q_stride, const int64_t* keys,
                         int m, int batch_pad, int max_len, int top_n, int32_t* d_in, void* hip_stream, void* lock);
// select: behind the forward, over d_logits [nq * m] and the keys the assembly left on the device; take: once the stream is drained
int rmu_rerank_select_(const float* d_logits, int64_t nq, int m, int top_n, int want_logits, void* hip_stream);
void rmu_rerank_take_(int64_t nq, int m, int top_n, int32_t* out_pos, float* out_scores, float* out_logits);
}
