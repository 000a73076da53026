// bert_plan.h -- which kernels one encoder forward runs (bert.hip launches them): the thresholds, the RMU_* switches that steer the choice,
// and the choice itself as a pure function of the call's shape.  Host-only plain C++ (no HIP type): tests/test_encoder_regimes_cpu.py holds
// enc_plan() against the table restated in tests/encoder_regimes.py over the whole shape domain, through rmu_bert_plan_ (bert.hip).
#pragma once
#include <stdint.h>

// ---- thresholds: tokens = batch * max_len (the upper bound `cap` of a call's packed tokens) unless named otherwise ------------------------
// Tokens up to which launch_gemm takes k_gemm_small, and from which the bulk QKV projection takes the persistent k_gemm3.  Round 4 measured
// the rerank shape (14 pairs, ~1.5k tokens, tools/ce_probe.py) with k_gemm_small over token blocks of 32 / 64 / 128 up to 4k-64k tokens and
// with deeper / smaller tiled configurations (128x128 x 3-4 stages, 64x128 x 4-6): nothing beat the round-3 choice (0.48-0.50 ms per call
// either way; every launch there is 5-15 us of latency, not of work), so the thresholds stay.  (The deeper / smaller configurations were
// selectable once, RMU_GEMM_CFG, and are retired.)  Debug builds keep the threshold knobs: RMU_MID_TOKENS, RMU_SMALL_TB, RMU_G3_MIN.
constexpr int SMALL_M = 256;
// ... and up to which QKV projection + attention are one launch (k_qkv_attn_small).  tools/small_ab.sh, one box, every output bit-identical:
// a 16-token query forward 0.182 ms fused / 0.183 apart (no gain: inside a replayed graph a kernel boundary is not the 4.4 us it costs under
// the profiler, a kernel's own load -> MFMA -> store chain is), the 14-pair rerank forward (1.5k tokens) 0.417 fused / 0.437 apart: the
// whole folded path takes it.
constexpr int QKV_ATTN_TOKENS = 2560;
// (round 6) ... but not below QKV_ATTN_MIN_TOKENS: one short query (16-48 tokens) runs 2.6-4.5 % faster on the two launches (a
// workgroup per (head, sequence) is 12 workgroups for one query), the 14-pair rerank call 3.7 % faster on the fused one
// (profiles/r06_ab_interactive.txt).  Bit-identical either way.
constexpr int QKV_ATTN_MIN_TOKENS = 128;
// The small path (a whole forward on k_gemm_small with the LayerNorms folded) up to this cap and this max_len.  Measured (tools/ce_probe.py,
// cross-encoder forward per call): 14 pairs / 1548 tokens 0.464-0.468 ms on the tiled kernels, 0.412-0.424 on the small path; 30 pairs /
// 3360 tokens (cap 4800: above the threshold) 0.50-0.51 tiled vs 0.65 small -- the fold pays up to ~2.5k tokens
constexpr int FOLD_TOKENS = 2560;
constexpr int FOLD_MAX_LEN = 256;
constexpr int CU_HERE_BATCH = 256;        // batch up to which (and cap <= FOLD_TOKENS) k_embed_ln<true> builds the sequence offsets itself
constexpr int EMBED_SEQ_BATCH = 512;      // batch from which the embedding is k_embed_ln_seq (a workgroup per sequence)
constexpr int KT4_MAX_LEN = 128;          // attention tile count KT: 4 up to this max_len,
constexpr int KT8_MAX_LEN = 256;          //   8 up to this one, 16 above (bulk only: the small path stops at FOLD_MAX_LEN)
// The fused FFN kernels give each 128-token tile to ONE workgroup, which then streams all 2.36 MB of FFN weights through one CU (~100 us
// per layer whatever the batch): below ~128 tiles most CUs would idle and the GEMM pair, whose feature tiles spread over the chip, is
// faster (measured: 8k tokens 0.82 vs 0.95 ms per forward, one 16-token query 0.44 vs 0.63 ms; 32k tokens 1.70 vs 1.45)
constexpr int FFN3_TOKENS = 16384;
constexpr int CTX_TILED_TOKENS = 32768;   // above: k_attn3 writes ctx as the 1-KiB operand blocks the out-proj GEMM's LDS-DMA reads whole
// k_gemm with few tiles (latency-bound: every workgroup walks K alone): 128 x 128 tiles in 64-k stages halve the stage count and double
// the workgroups -- 4k tokens 0.70 -> 0.60 ms per forward, 16k tokens 1.12 -> 1.07; above this, 256 x 128 / 32-k stages (best of the
// seven tile / stage / ring combinations measured in round 2)
constexpr int GEMM_T128_TOKENS = 32768;
// rmu_bert_encode_host / rmu_bert_search_mmr carry up to HOST_TOKENS tokens (batch * max_len): one query, or the <= 14 (query, passage)
// pairs of one rerank call (server/ScoredCrossEncoderReranker.py:42) -- and give back at most HOST_ROWS rows of 384 floats (pooled
// vectors / the token states of a 256-token call) or one logit per sequence
constexpr int HOST_TOKENS = 4096;
constexpr int HOST_ROWS = 256;

// ---- every RMU_* switch that steers the forward, at its default.  enc_switches() (bert.hip) fills it once per process,
// through rmu_env only: nothing here is honoured without RMU_TUNING=1.
struct EncSwitches {
    bool small_fuse = true;                         // RMU_SMALL_FUSE=0: the separate k_cu_seqlens launch at the interactive sizes too
    bool embed_seq = true;                          // RMU_EMBED_SEQ=0: a wave per (sequence, position) slot at every batch
    bool gemm_small = true;                         // RMU_GEMM_SMALL=0: no k_gemm_small, hence no small path
    bool ln_fuse = true;                            // RMU_LN_FUSE=0: no folded LayerNorms, hence no small path
    int64_t fold_tokens = FOLD_TOKENS;              // RMU_FOLD_TOKENS (0 = the tiled kernels from the first token on)
    int64_t qkv_attn_tokens = QKV_ATTN_TOKENS;      // RMU_QKV_ATTN_TOKENS (0 keeps QKV projection and attention apart)
    int64_t qkv_attn_min = QKV_ATTN_MIN_TOKENS;     // RMU_QKV_ATTN_MIN (0: fused from the first token on)
    bool qa = false;                                // RMU_QA=1: k_qa, see enc_plan
    int gemm3 = 1;                                  // RMU_GEMM3: k_gemm3 for: bit 0 QKV (default: 1.22 vs 1.38 ms), bit 1 out-proj (0.67 vs 0.61), bit 2 FFN1 + FFN2 instead of a fused FFN kernel (3.6 vs 3.35)
    bool qkv_hm = true;                             // RMU_QKV_HM=0: QKV row-major
    bool ctx_tiled = true;                          // RMU_CTX_TILED=0: ctx row-major
    int fused_ffn = -1;                             // RMU_FUSED_FFN=0 / 1 forces the GEMM pair / the fused FFN kernel at every size
    int ffn_v = 3;                                  // RMU_FFN_V=2: k_ffn2 (one wave per SIMD) instead of k_ffn3 (two)
    bool ffn_lnin = true;                           // RMU_FFN_LNIN=0: LayerNorm 1 as a separate k_layernorm launch
    bool h_tiled = true;                            // RMU_H_TILED=0: h row-major between layers
    int ffn_gelu = 0;                               // RMU_FFN_GELU=1: k_ffn2 with the scalar v_fma_f32 polynomial (A/B measurement)
    int ffn_pf = 4;                                 // RMU_FFN_PF=8: k_ffn2 with eight weight fragments read ahead (A/B measurement)
    int qa_dbg = 0;                                 // RMU_QA_DBG: k_qa's ablation flags
#ifdef RMU_DEBUG_KERNELS
    int64_t mid_tokens = SMALL_M;                   // RMU_MID_TOKENS (at least SMALL_M): launch_gemm takes k_gemm_small up to here
    int64_t g3_min = SMALL_M;                       // RMU_G3_MIN (at least mid_tokens): k_gemm3 / k_qa above
    int small_tb = 128;                             // RMU_SMALL_TB: launch_gemm's k_gemm_small token block (a multiple of 32)
#else
    static constexpr int64_t mid_tokens = SMALL_M, g3_min = SMALL_M;
    static constexpr int small_tb = 128;
#endif
};
const EncSwitches& enc_switches();

// ---- the plan of one forward.  rmu_bert_plan_ (bert.hip) writes the fields out as int32 in this order (enums by value, flags 0 / 1):
//   offsets_fused, embed, path, qkv, attn_kt, gemm, out_proj, ffn, ffn_ln_in, ctx_tiled, h_tiled, qkv_head_major, tq, th, tf
constexpr int ENC_PLAN_FIELDS = 15;
enum class EncEmbed : int32_t { Wave, Seq };              // k_embed_ln (a wave per (sequence, position) slot), k_embed_ln_seq (a workgroup per sequence)
enum class EncPath : int32_t { Small, Bulk };
enum class EncQkv : int32_t { GemmSmall, AttnSmall, Gemm, Gemm3, Qa };   // Gemm: through launch_gemm, in the form `gemm`
enum class EncGemm : int32_t { Small, T128, T256 };       // k_gemm_small, k_gemm on 128-row tiles, on 256-row tiles
enum class EncOutProj : int32_t { Gemm3, TiledA, Plain }; // k_gemm3, k_gemm reading ctx (and a tiled h) as operand blocks, launch_gemm
enum class EncFfn : int32_t { GemmSmall, PairLn, Gemm3Pair, Ffn2, Ffn3 };   // PairLn: k_layernorm, two launch_gemm, k_layernorm
struct EncPlan {
    bool offsets_fused;        // the sequence offsets come out of the embedding launch (k_embed_ln<true>), not out of k_cu_seqlens
    EncEmbed embed;
    EncPath path;
    EncQkv qkv;                // (Qa also needs the model's work list: the launch code falls back to Gemm3 without one)
    int attn_kt;               // 4, 8 or 16 tiles of 32 keys
    EncGemm gemm;              // what launch_gemm takes at this cap, wherever the bulk path goes through it
    EncOutProj out_proj;       // bulk
    EncFfn ffn;
    bool ffn_ln_in;            // Ffn2 / Ffn3: LayerNorm 1 in the kernel's prologue (no k_layernorm launch in the layer)
    bool ctx_tiled;
    bool h_tiled;              // h travels tiled BETWEEN layers: layer li of `layers` writes it tiled iff li < layers (the last one feeds the heads)
    bool qkv_head_major;       // the stride between (part, head) planes is the workspace's token capacity: the launch code knows it
    int tq, th, tf;            // small path: tokens per k_gemm_small workgroup of the QKV / 384-wide / FFN1 launches
};

// Pure: the same shape and switches give the same plan.  `layers` only decides whether there is a "between layers" for h_tiled.
inline EncPlan enc_plan(int batch, int max_len, int layers, const EncSwitches& sw) {
    const int64_t cap = (int64_t)batch * max_len;
    EncPlan p{};
    // (round 5) the interactive sizes: the sequence offsets are built inside k_embed_ln
    p.offsets_fused = sw.small_fuse && batch <= CU_HERE_BATCH && cap <= FOLD_TOKENS;
    p.embed = !p.offsets_fused && sw.embed_seq && batch >= EMBED_SEQ_BATCH ? EncEmbed::Seq : EncEmbed::Wave;
    p.attn_kt = max_len <= KT4_MAX_LEN ? 4 : max_len <= KT8_MAX_LEN ? 8 : 16;
    p.gemm = sw.gemm_small && cap <= sw.mid_tokens ? EncGemm::Small : cap <= GEMM_T128_TOKENS ? EncGemm::T128 : EncGemm::T256;
    if (cap <= sw.fold_tokens && max_len <= FOLD_MAX_LEN && sw.gemm_small && sw.ln_fuse) {
        p.path = EncPath::Small;
        // (round 5) QKV projection and attention as ONE launch (k_qkv_attn_small: a workgroup per (head, sequence); bit-identical to the pair)
        p.qkv = cap <= sw.qkv_attn_tokens && cap > sw.qkv_attn_min ? EncQkv::AttnSmall : EncQkv::GemmSmall;
        p.out_proj = EncOutProj::Plain;
        p.ffn = EncFfn::GemmSmall;
        // Token blocks per workgroup: enough of them to fill the chip, few enough to amortise the weight rows a workgroup keeps in registers
        // (N / 32 feature blocks x cap / tb token blocks ~ 256-512 workgroups): ~384 workgroups in all, a multiple of 32, at least 32
        auto tb_for = [cap](int n_feature_blocks) {
            const int64_t blocks = 384 / n_feature_blocks > 1 ? 384 / n_feature_blocks : 1;
            const int64_t tb = ((cap + blocks - 1) / blocks + 31) / 32 * 32;
            return (int)(tb < 32 ? 32 : tb > 1024 ? 1024 : tb);
        };
        p.tq = tb_for(3 * 384 / 32), p.th = tb_for(384 / 32), p.tf = tb_for(1536 / 32);
        return p;
    }
    p.path = EncPath::Bulk;
    const bool g3_qkv = (sw.gemm3 & 1) && cap > sw.g3_min;
    // (round 6) RMU_QA=1: QKV projection + attention as ONE launch per layer (k_qa) for sequences up to 256 tokens.  Built, bit-identical to
    // k_gemm3 + k_attn3 (tests), and NOT the default: 2.31 ms per layer in its lockstep form, 2.99 as a ping-pong of the two wave halves,
    // against 1.90 for the pair -- at 8 waves per CU (the 96 token-fragment registers) one wave's attention chain takes ~6.6k cycles per
    // head whatever runs beside it (profiles/r06_qa_fusion.md)
    p.qkv = sw.qa && g3_qkv && max_len <= 256 && batch <= 65536 ? EncQkv::Qa : g3_qkv ? EncQkv::Gemm3 : EncQkv::Gemm;
    // QKV head-major when k_gemm3 writes it and k_attn3 reads it
    p.qkv_head_major = sw.qkv_hm && g3_qkv;
    p.ctx_tiled = sw.ctx_tiled && !(sw.gemm3 & 2) && cap > CTX_TILED_TOKENS;
    p.out_proj = (sw.gemm3 & 2) ? EncOutProj::Gemm3 : p.ctx_tiled ? EncOutProj::TiledA : EncOutProj::Plain;
    const bool fused_ffn = !(sw.gemm3 & 4) && (sw.fused_ffn < 0 ? cap > FFN3_TOKENS : sw.fused_ffn != 0);
    p.ffn = (sw.gemm3 & 4) ? EncFfn::Gemm3Pair : !fused_ffn ? EncFfn::PairLn : sw.ffn_v == 3 ? EncFfn::Ffn3 : EncFfn::Ffn2;
    // k_ffn3 (default; two waves per SIMD) and k_ffn2 (one) also take LayerNorm 1 into their prologue: the out-proj sum y goes straight in
    p.ffn_ln_in = fused_ffn && sw.ffn_lnin;
    // Between layers h travels TILED (1-KiB blocks of 16 tokens x 32 features: the next QKV GEMM's A pieces and the next out-proj's
    // residual pieces become whole contiguous KiB); the last layer writes row-major for the pooling heads.
    p.h_tiled = sw.h_tiled && p.ffn == EncFfn::Ffn3 && p.ffn_ln_in && p.ctx_tiled && (sw.gemm3 & 1) && layers > 1;
    return p;
}
