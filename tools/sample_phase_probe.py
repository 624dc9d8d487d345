#!/usr/bin/env python3
"""Where the sampling kernel's time goes, by differential timing of the single op
(runtime.sample -> inferd_sample, the product kernel; 16 rows of randn * 3 bf16 logits, T 0.6,
top-p 0.95): back-to-back launches between two events, per configuration --
  V = 48,     k = 20   fewer tiles than k: no tau search (B); 48 candidates ranked (D), the draw (E)
  V = 1024,   k = 20   + the 16-round tau search over 64 tile maxima (B)
  V = 151936, k = 1/20/64   + 9,496 tile maxima per row (A: here computed from the logits; the span
                       reads the GEMV's keys instead) and the candidate tiles' read-back (C); k moves D
Writes profiles/sample_phase_probe.json (us per launch) and prints it.
    python tools/sample_phase_probe.py [--reps 400] [--out profiles/sample_phase_probe.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=400)
    p.add_argument("--rows", type=int, default=16)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_phase_probe.json"))
    args = p.parse_args()
    from inferd_amd.ops import ops as T
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    out = {}
    for vocab, k in ((48, 20), (1024, 20), (151936, 1), (151936, 20), (151936, 64)):
        lg = (torch.randn(args.rows, vocab, generator=g) * 3).to(torch.bfloat16).to(dev)
        pos = torch.arange(args.rows, dtype=torch.int32, device=dev)
        ids = torch.empty(args.rows, dtype=torch.int32, device=dev)

        def launch():
            T.sample(lg, 0.6, k, 0.95, 1234, None, pos, ids, None, None)
        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        out[f"V{vocab}_k{k}"] = round(e0.elapsed_time(e1) / args.reps * 1e3, 2)
    res = {"tool": "tools/sample_phase_probe.py", "device": torch.cuda.get_device_name(dev),
           "what": "single op inferd_sample on randn * 3 bf16 logits, T 0.6, top-p 0.95, back-to-back launches "
                   "between two events (the floor includes the host's launch pace)",
           "rows": args.rows, "reps": args.reps, "us_per_launch": out}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
