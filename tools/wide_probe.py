"""The wide exact scan (scan_wide_kernel: queries streamed through the LDS ring) next to the register-resident scan, in ONE process:
a corpus of --rows unit-norm rows at width 768 twice -- through scan_topk_kernel (the product kernel, screening off) and through
scan_wide_kernel (RMU_OPT_WIDE_SCAN) -- and at 1024, 1536 and 3072, where only the wide kernel exists; batches 1, 32 and 1024, k = 10.

Per shape: the step time (device queries and outputs on a caller stream, nothing synchronises inside a window of calls between two
device events; median of --reps windows) and the hipEvent time of the scan kernel alone (rmu_last_scan_ms, median of --reps calls).
Fractions of the kernel time: of 8 TB/s on the rows' bytes (n * dpad * 4) and of the 157.3 TF/s f32 MFMA roof on 2 * n * dpad * B flop.
Then the two comparisons DESIGN.md 4.1b quotes: forced-wide over product at 768, and every wide width over forced-wide 768 per byte
(batch 1) and per flop (batch 1024).

  python tools/wide_probe.py [--rows 1000000] [--widths 768,1024,1536,3072] [--batches 1,32,1024] [--k 10] [--window 0.3] [--reps 3]
                             [--out profiles/wide_scan.md]

Prints one JSON line; --out also writes the table as markdown."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragmeup_amd import FlatIndex  # noqa: E402

HBM_BYTES_PER_S = 8e12
MFMA_F32_FLOPS = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--widths", default="768,1024,1536,3072")
    ap.add_argument("--batches", default="1,32,1024")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the markdown table here (e.g. profiles/wide_scan.md)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_probe: no GPU: there is nothing to measure without one")
    dev = torch.device("cuda", 0)
    widths = [int(v) for v in a.widths.split(",")]
    batches = [int(v) for v in a.batches.split(",")]
    stream = torch.cuda.Stream()

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls          # ms per call

    results = []
    for dim in widths:
        dpad = 192 if dim <= 192 else 384 if dim <= 384 else 768 if dim <= 768 else (dim + 63) // 64 * 64
        idx = FlatIndex(dim, capacity_hint=a.rows, device=0)
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        step = 1 << 17
        for lo in range(0, a.rows, step):
            x = torch.randn((min(a.rows, lo + step) - lo, dim), generator=g, dtype=torch.float32, device=dev)
            x /= x.norm(dim=1, keepdim=True)
            idx.add(x)
        del x
        idx.set_screening(False)
        q_all = torch.randn((max(batches), dim), generator=g, dtype=torch.float32, device=dev)
        q_all /= q_all.norm(dim=1, keepdim=True)
        torch.cuda.synchronize()
        for kernel in (["scan_topk_kernel", "scan_wide_kernel"] if dim <= 768 else ["scan_wide_kernel"]):
            idx.set_wide_scan(kernel == "scan_wide_kernel" and dim <= 768)
            for b in batches:
                q = q_all[:b].contiguous()
                out = (torch.empty((b, a.k), dtype=torch.float32, device=dev), torch.empty((b, a.k), dtype=torch.int64, device=dev))
                fn = lambda: idx.search(q, a.k, stream=stream.cuda_stream, out=out)
                for _ in range(2):
                    window(fn, 2)
                calls = max(3, int(a.window * 1e3 / max(window(fn, 3), 1e-3)))
                step_ms = statistics.median(window(fn, calls) for _ in range(a.reps))
                idx.set_timing(True)                 # the kernel alone: events around the scan launch on the library's own stream
                kern = []
                for _ in range(a.reps + 1):
                    idx.search(q, a.k, out=out)
                    kern.append(idx.last_scan_ms())
                idx.set_timing(False)
                kern_ms = statistics.median(kern[1:])
                geo = idx.last_geometry()
                nbytes = a.rows * dpad * 4
                flop = 2.0 * a.rows * dpad * b
                results.append({"dim": dim, "dpad": dpad, "kernel": kernel, "batch": b, "step_ms": round(step_ms, 5), "scan_ms": round(kern_ms, 5),
                                "hbm_fraction": round(nbytes / (kern_ms * 1e-3) / HBM_BYTES_PER_S, 4),
                                "mfma_fraction": round(flop / (kern_ms * 1e-3) / MFMA_F32_FLOPS, 4), "grid": geo["grid"], "lds_bytes": geo["lds_bytes"]})
        idx.close()
        del idx
        torch.cuda.empty_cache()

    def pick(dim, kernel, b):
        for r in results:
            if (r["dim"], r["kernel"], r["batch"]) == (dim, kernel, b):
                return r
        return None

    ratios = {"forced_wide_over_product_768": {}, "per_byte_b1_over_forced_768": {}, "per_flop_b1024_over_forced_768": {}}
    for b in batches:
        p, w = pick(768, "scan_topk_kernel", b), pick(768, "scan_wide_kernel", b)
        if p and w:
            ratios["forced_wide_over_product_768"][str(b)] = round(w["scan_ms"] / p["scan_ms"], 4)
    for key, b in (("per_byte_b1_over_forced_768", 1), ("per_flop_b1024_over_forced_768", 1024)):
        base = pick(768, "scan_wide_kernel", b)
        for dim in widths:
            r = pick(dim, "scan_wide_kernel", b)
            if base and r and dim > 768:
                ratios[key][str(dim)] = round((r["scan_ms"] / r["dpad"]) / (base["scan_ms"] / base["dpad"]), 4)
    doc = {"probe": "wide_scan", "rows": a.rows, "k": a.k, "window_s": a.window, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "results": results, "ratios": ratios}
    print(json.dumps(doc), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(f"# Wide exact scan: tools/wide_probe.py, {a.rows} rows, k = {a.k}, {doc['device']}\n\n")
            fh.write("step = one search on a caller stream (median of %d windows of %.1f s); scan = hipEvent time of the scan kernel alone; "
                     "HBM = rows' bytes / scan / 8 TB/s; MFMA = 2 n dpad B / scan / 157.3 TF/s.\n\n" % (a.reps, a.window))
            fh.write("| dim | dpad | kernel | batch | step ms | scan ms | HBM | MFMA | grid | LDS bytes |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in results:
                fh.write("| %d | %d | %s | %d | %.4f | %.4f | %.3f | %.3f | %d | %d |\n" % (
                    r["dim"], r["dpad"], r["kernel"], r["batch"], r["step_ms"], r["scan_ms"], r["hbm_fraction"], r["mfma_fraction"], r["grid"], r["lds_bytes"]))
            fh.write("\nscan_wide_kernel over scan_topk_kernel at 768 (scan ms), by batch: %s\n\n" % json.dumps(ratios["forced_wide_over_product_768"]))
            fh.write("scan ms per byte at batch 1, over forced-wide 768: %s\n\n" % json.dumps(ratios["per_byte_b1_over_forced_768"]))
            fh.write("scan ms per flop at batch 1024, over forced-wide 768: %s\n" % json.dumps(ratios["per_flop_b1024_over_forced_768"]))


if __name__ == "__main__":
    main()
