// bert_any.h -- the general BERT forward (bert_any.hip: head width 64, hidden 128..1024, ffn 64..4096) as bert.hip sees it: an opaque
// context behind `struct rmu_bert`, created, sized, run and released through the functions below.  Internal symbols (trailing underscore).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rmu.h"

struct rmu_any_bert;

// hidden = 64 * heads with 2 <= heads <= 16, ffn a multiple of 64 in [64, 4096]; 384/12/1536 is NOT general (it has its own kernels).  No HIP call.
bool rmu_any_geometry_(const rmu_bert_cfg* cfg);
// converts the weights (DEVICE fp32, the order of ragmeup_amd/bert.py: weight_order) on stream s; the caller drains s and checks it
int rmu_any_create_(rmu_any_bert** out, const rmu_bert_cfg* cfg, const void* const* wptr, hipStream_t s);
void rmu_any_free_(rmu_any_bert* a);
// true when rmu_any_ensure_ws_ would release a buffer: the caller first waits for whatever still uses the workspace
bool rmu_any_ws_grows_(const rmu_any_bert* a, int batch, int max_len);
int rmu_any_ensure_ws_(rmu_any_bert* a, int batch, int max_len);
// every launch of one forward on stream s (device pointers; no allocation, no synchronisation)
void rmu_any_enqueue_forward_(rmu_any_bert* a, const int32_t* ids, const int32_t* type_ids, const int32_t* lens, int batch, int max_len, int mode,
                              float* out_dev, int64_t out_stride, hipStream_t s);
