"""The general encoder (csrc/bert_any.hip: BERTs with 64-wide heads) beside what a user would otherwise run on this GPU -- transformers'
BertModel under PyTorch-ROCm, bf16 and fp32 -- on the same weights and the same batches, alternated in ONE process.

Models: BERT-base (768/12/3072, 12 layers) and BERT-large (1024/16/4096, 24 layers), random weights.
  bulk   8192 chunks, lengths ~ clip(N(128, 32), 16, 256), embedded in the batches MI355XEmbeddings forms (length-sorted, 1 Mi padded
         tokens each): chunks/s and ms per forward;
  query  one sequence of 16 tokens: latency.
Every timed window is taken between two device events around synchronised work, lasts at least --window seconds, and follows a warm-up of
every shape it uses; the three engines take turns for --rounds rounds (median, and min .. max as the run-to-run spread of this call).
FLOPs are counted from the shapes (2 * m * n * k per GEMM, 4 * len^2 * hidden per layer for the two attention products) and set against
the 2.5 PF/s dense bf16 MFMA peak: for the whole forward that is an end-to-end figure, not a kernel's share.

  python tools/anybert_probe.py [--chunks 8192] [--window 1.0] [--rounds 3] [--out profiles/anybert_encoder.md] [--json anybert_probe.json]
  python tools/anybert_probe.py --trace base|large [--forwards 3]       # the bulk forwards alone, to run under rocprofv3 --kernel-trace --stats
  python tools/anybert_probe.py --kernel-stats <kernel_stats.csv> --model base|large --forwards N --out profiles/anybert_encoder.md
        # no GPU work: folds the profiler's per-kernel times and the shape-derived FLOPs into the per-kernel table of the markdown file

Finds a GPU or fails (the --kernel-stats form reads files only)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BF16 = 2.5e15
MODELS = {"base": (768, 12, 3072, 12), "large": (1024, 16, 4096, 24)}
VOCAB = 30522


def make_weights(hidden, heads, ffn, layers, seed=0):
    """HF name -> fp32 numpy, N(0, 0.02) Linear / embedding weights, perturbed LayerNorms and biases"""
    from ragmeup_amd.bert import weight_order
    rng = np.random.default_rng(seed)
    w = {}
    for name in weight_order(layers, False):
        if name.endswith("embeddings.weight"):
            rows = {"word": VOCAB, "position": 512, "token_type": 2}[name.split(".")[1].split("_embeddings")[0]]
            w[name] = (0.02 * rng.standard_normal((rows, hidden))).astype(np.float32)
        elif "LayerNorm.weight" in name:
            w[name] = (1 + 0.05 * rng.standard_normal(hidden)).astype(np.float32)
        elif name.endswith(".bias"):
            n = ffn if "intermediate" in name else hidden
            w[name] = (0.05 * rng.standard_normal(n)).astype(np.float32)
        else:
            o, i = (ffn, hidden) if "intermediate" in name else (hidden, ffn) if name.endswith("output.dense.weight") and "attention" not in name \
                else (hidden, hidden)
            w[name] = (0.02 * rng.standard_normal((o, i))).astype(np.float32)
    return w


def synth_tokens(n, seed=7, lmin=16, lmax=256, mean=128, std=32):
    rng = np.random.default_rng(seed)
    lens = np.clip(np.rint(rng.normal(mean, std, n)), lmin, lmax).astype(np.int32)
    ids = np.zeros((n, int(lens.max())), dtype=np.int32)
    for i, l in enumerate(lens):
        ids[i, :l] = rng.integers(1000, VOCAB, l)
        ids[i, 0], ids[i, l - 1] = 101, 102
    return ids, lens


def forward_flops(lens, hidden, ffn, layers):
    """(GEMM flops, attention flops) of one forward over sequences of these lengths"""
    lens = np.asarray(lens, dtype=np.float64)
    gemm = 2.0 * lens.sum() * (4 * hidden * hidden + 2 * hidden * ffn) * layers
    attn = 4.0 * (lens ** 2).sum() * hidden * layers
    return gemm, attn


def batches(lens, token_budget=1 << 20):
    """MI355XEmbeddings._batches: length-sorted index arrays under a padded-token budget"""
    order = np.argsort(-lens, kind="stable")
    i = 0
    while i < len(order):
        L = int(lens[order[i]])
        n = max(1, min(len(order) - i, token_budget // max(L, 1), 65535))
        yield order[i:i + n]
        i += n


def hf_model(w, hidden, heads, ffn, layers, dtype, dev):
    import torch
    from transformers import BertConfig, BertModel
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=ffn,
                     max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")
    m = BertModel(cfg, add_pooling_layer=False)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected, unexpected
    return m.to(dev, dtype).eval()


def run_probe(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("anybert_probe: no GPU: there is nothing to measure without one")
    from ragmeup_amd.bert import MODE_MEAN, BertEncoder
    dev = torch.device("cuda", 0)
    ids, lens = synth_tokens(a.chunks)
    q_ids, q_lens = synth_tokens(1, seed=3, lmin=16, lmax=16, mean=16, std=1)
    groups = [idx for idx in batches(lens)]
    result = {"chunks": a.chunks, "tokens": int(lens.sum()), "batches": [[len(g), int(lens[g[0]])] for g in groups], "window_s": a.window,
              "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "models": {}}

    def timed(fn):
        """fn() enqueues AND synchronises one unit of work; windows of at least a.window seconds -> ms per unit"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n, t0 = 0, time.perf_counter()
        e0.record()
        while True:
            fn()
            n += 1
            if time.perf_counter() - t0 >= a.window:
                break
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for name in a.models.split(","):
        hidden, heads, ffn, layers = MODELS[name]
        w = make_weights(hidden, heads, ffn, layers)
        enc = BertEncoder(w, layers=layers, heads=heads, ffn=ffn)
        d_batches = [(torch.as_tensor(ids[g, :int(lens[g[0]])], device=dev).contiguous(), torch.as_tensor(lens[g], device=dev).contiguous()) for g in groups]
        outs = [torch.empty((len(g), hidden), device=dev) for g in groups]
        dq = (torch.as_tensor(q_ids, device=dev).contiguous(), torch.as_tensor(q_lens, device=dev).contiguous())
        oq = torch.empty((1, hidden), device=dev)
        cur = torch.cuda.current_stream(dev)

        def ours_bulk():
            for (bi, bl), o in zip(d_batches, outs):
                enc.encode_ids(bi, bl, None, mode=MODE_MEAN, out=o, stream=cur)
            cur.synchronize()

        def ours_query():
            enc.encode_ids(dq[0], dq[1], None, mode=MODE_MEAN, out=oq, stream=cur)
            cur.synchronize()

        engines = {"ours": (ours_bulk, ours_query)}
        for tag, dtype in (("torch_bf16", torch.bfloat16), ("torch_fp32", torch.float32)):
            m = hf_model(w, hidden, heads, ffn, layers, dtype, dev)
            masks = [(torch.arange(bi.shape[1], device=dev)[None] < bl[:, None]).to(torch.int64) for bi, bl in d_batches]
            t_ids = [bi.to(torch.int64) for bi, _ in d_batches]
            qi, qm = dq[0].to(torch.int64), torch.ones((1, 16), dtype=torch.int64, device=dev)

            def pooled(model, i, mk):
                with torch.no_grad():
                    h = model(input_ids=i, attention_mask=mk).last_hidden_state.float()
                    f = mk.unsqueeze(-1).float()
                    return torch.nn.functional.normalize((h * f).sum(1) / f.sum(1).clamp(min=1e-9), p=2, dim=1)

            def t_bulk(model=m, t_ids=t_ids, masks=masks):
                res = [pooled(model, i, mk) for i, mk in zip(t_ids, masks)]
                torch.cuda.synchronize(dev)
                return res

            def t_query(model=m, qi=qi, qm=qm):
                r = pooled(model, qi, qm)
                torch.cuda.synchronize(dev)
                return r
            engines[tag] = (t_bulk, t_query)

        # agreement first (also the warm-up of every shape): ours against the fp32 baseline, chunk by chunk
        ours_bulk()
        ref = engines["torch_fp32"][0]()
        cos = min(float((o * r).sum(1).min()) for o, r in zip(outs, ref))
        for tag, (fb, fq) in engines.items():
            fb(); fq(); fq()
        bulk = {tag: [] for tag in engines}
        query = {tag: [] for tag in engines}
        for _ in range(a.rounds):
            for tag, (fb, fq) in engines.items():
                bulk[tag].append(timed(fb))
            for tag, (fb, fq) in engines.items():
                query[tag].append(timed(fq))
        gemm, attn = forward_flops(lens, hidden, ffn, layers)
        entry = {"geometry": [hidden, heads, ffn, layers], "min_cos_vs_torch_fp32": cos, "gemm_flop": gemm, "attn_flop": attn, "engines": {}}
        for tag in engines:
            ms = statistics.median(bulk[tag])
            entry["engines"][tag] = {
                "bulk_ms": ms, "bulk_ms_min": min(bulk[tag]), "bulk_ms_max": max(bulk[tag]), "ms_per_forward": ms / len(groups),
                "chunks_per_s": a.chunks / ms * 1e3, "chunks_per_s_min": a.chunks / max(bulk[tag]) * 1e3, "chunks_per_s_max": a.chunks / min(bulk[tag]) * 1e3,
                "end_to_end_tflops": (gemm + attn) / ms / 1e9, "end_to_end_of_peak": (gemm + attn) / (ms * 1e-3) / PEAK_BF16,
                "query_ms": statistics.median(query[tag]), "query_ms_min": min(query[tag]), "query_ms_max": max(query[tag])}
        result["models"][name] = entry
        print(json.dumps({name: entry}), flush=True)
        enc.close()
        del engines, d_batches, outs
        torch.cuda.empty_cache()
    return result


def run_trace(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("anybert_probe: no GPU: there is nothing to trace without one")
    from ragmeup_amd.bert import MODE_MEAN, BertEncoder
    hidden, heads, ffn, layers = MODELS[a.trace]
    enc = BertEncoder(make_weights(hidden, heads, ffn, layers), layers=layers, heads=heads, ffn=ffn)
    ids, lens = synth_tokens(a.chunks)
    for _ in range(a.forwards):
        for g in batches(lens):
            enc.encode_ids(ids[g, :int(lens[g[0]])], lens[g], None, mode=MODE_MEAN)
    enc.close()
    print(json.dumps({"traced": a.trace, "forwards": a.forwards, "chunks": a.chunks}))


def kernel_table(a):
    """rocprofv3's kernel_stats.csv (Name, Calls, TotalDurationNs, ...) -> markdown rows with the shape-derived share of the bf16 peak"""
    hidden, heads, ffn, layers = MODELS[a.model]
    _, lens = synth_tokens(a.chunks)
    gemm, attn = forward_flops(lens, hidden, ffn, layers)
    toks = float(lens.sum())
    per = {"EPI_BIAS": 2 * toks * 3 * hidden * hidden * layers, "EPI_GELU": 2 * toks * hidden * ffn * layers,
           "EPI_RESID": 2 * toks * (hidden * hidden + hidden * ffn) * layers}
    rows = []
    with open(a.kernel_stats, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "k_any_" not in name and "k_gemm_any" not in name:
                continue
            total_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            calls = int(float(r.get("Calls") or 0))
            flop = None
            if "k_gemm_any<0>" in name or "k_gemm_anyILi0" in name:
                flop = per["EPI_BIAS"]
            elif "k_gemm_any<1>" in name or "k_gemm_anyILi1" in name:
                flop = per["EPI_GELU"]
            elif "k_gemm_any<2>" in name or "k_gemm_anyILi2" in name:
                flop = per["EPI_RESID"]
            elif "k_any_attn" in name:
                flop = attn
            ms = total_ns / 1e6 / a.forwards
            share = f"{flop / (ms * 1e-3) / PEAK_BF16 * 100:.1f} %" if flop else "-"
            tf = f"{flop / ms / 1e9:.0f}" if flop else "-"
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows.append((ms, f"| `{short}` | {calls // a.forwards} | {ms:.3f} | {tf} | {share} |"))
    rows.sort(reverse=True)
    total = sum(ms for ms, _ in rows)
    head = [f"\n## Per-kernel times, {a.model} ({hidden}/{heads}/{ffn}, {layers} layers), one bulk pass over {a.chunks} chunks",
            "", f"From a separate `rocprofv3 --kernel-trace --stats` run of `--trace {a.model} --forwards {a.forwards}` (tracing slows the host: times of",
            "kernels only).  FLOPs from the shapes; share = achieved rate over the 2.5 PF/s dense bf16 MFMA peak.", "",
            "| kernel | launches per pass | ms per pass | TFLOP/s | share of bf16 peak |", "|---|---|---|---|---|"]
    text = "\n".join(head + [r for _, r in rows] + [f"| all kernels of the forward | | {total:.3f} | | |", ""])
    with open(a.out, "a") as f:
        f.write(text)
    print(text)


def write_markdown(res, path):
    L = ["# The general encoder (bert_any.hip) beside transformers + PyTorch-ROCm", "",
         f"`tools/anybert_probe.py`, one process on one {res['device']}: {res['chunks']} chunks ({res['tokens']} tokens, lengths ~ clip(N(128, 32), 16, 256))",
         f"embedded in {len(res['batches'])} length-sorted batches of at most 1 Mi padded tokens ({', '.join(f'{n} x {l}' for n, l in res['batches'])}); one query of",
         f"16 tokens.  Same random weights and the same batches for every engine; the engines take turns for {res['rounds']} rounds of windows of at least",
         f"{res['window_s']} s between two device events around synchronised work, after a warm-up of every shape.  Median (min .. max of the rounds: the",
         "run-to-run spread of this call).  `end-to-end` = shape-derived FLOPs of the forward (GEMMs + the two attention products) over the wall time of",
         "the whole pass, against the 2.5 PF/s dense bf16 MFMA peak: a whole-program figure, not a kernel's share.", ""]
    for name, e in res["models"].items():
        h, nh, ff, ly = e["geometry"]
        L += [f"## {name}: {h}/{nh}/{ff}, {ly} layers", "",
              f"Agreement: minimum cosine of ours against the torch fp32 embedding over all chunks {e['min_cos_vs_torch_fp32']:.6f}.", "",
              "| engine | chunks/s | ms per bulk pass | ms per forward | end-to-end TFLOP/s | of bf16 peak | one 16-token query, ms |", "|---|---|---|---|---|---|---|"]
        for tag, r in e["engines"].items():
            L.append(f"| {tag} | {r['chunks_per_s']:.0f} ({r['chunks_per_s_min']:.0f} .. {r['chunks_per_s_max']:.0f}) | {r['bulk_ms']:.1f} | {r['ms_per_forward']:.1f} | "
                     f"{r['end_to_end_tflops']:.0f} | {r['end_to_end_of_peak'] * 100:.1f} % | {r['query_ms']:.3f} ({r['query_ms_min']:.3f} .. {r['query_ms_max']:.3f}) |")
        o, t = e["engines"]["ours"], e["engines"]["torch_bf16"]
        ratio = o["chunks_per_s"] / t["chunks_per_s"]
        spread = max((r["chunks_per_s_max"] - r["chunks_per_s_min"]) / r["chunks_per_s"] for r in (o, t))
        verdict = "no lower than the torch bf16 baseline by more than the spread" if ratio >= 1 - spread else "LOWER than the torch bf16 baseline by more than the spread"
        L += ["", f"Bulk rate, ours over torch bf16: {ratio:.2f}x (largest spread of the two in this call: {spread * 100:.1f} %): {verdict}.",
              f"One query, ours over torch bf16: {t['query_ms'] / o['query_ms']:.2f}x faster." if o["query_ms"] <= t["query_ms"] else
              f"One query, ours over torch bf16: {o['query_ms'] / t['query_ms']:.2f}x slower.", ""]
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8192)
    ap.add_argument("--models", default="base,large")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", default=None, choices=list(MODELS))
    ap.add_argument("--forwards", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--model", default="base", choices=list(MODELS))
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_table(a)
    if a.trace:
        return run_trace(a)
    res = run_probe(a)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)
    if a.out:
        write_markdown(res, a.out)
    print(json.dumps({"anybert_probe": {m: {t: round(r["chunks_per_s"]) for t, r in e["engines"].items()} for m, e in res["models"].items()}}))


if __name__ == "__main__":
    main()
