#!/usr/bin/env python3
"""What a sampled decode step costs over a greedy one: Qwen3-8B, B = 16 at 2k context, the decode
loop of bench.py's headline (pipeline.PipelineStage over one span: a DecodeGraph whose next_ids
feed ids), once with the greedy head and once with the sampled head (temperature 0.6, top-k 20,
top-p 0.95 -- the reference client's defaults, qwen3_config.py:5-7).

The two modes alternate greedy, sampled, sampled, greedy, ... on one prefilled state (the context
grows by a few tokens per run; the mirrored order cancels that drift in the means).  Every run is
W warm-up and K timed steps between two HIP events on the launch stream, then a few eager
event-instrumented steps for the lm_head class time (INFERD_PROF_LMHEAD: final norm + lm_head GEMV
+ argmax reduce or the sampling kernel).  Writes profiles/sample_bench.json:

    python tools/sample_bench.py [--rounds 3] [--steps 64] [--warmup 8] [--out profiles/sample_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLING = (0.6, 20, 0.95)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="qwen3-8b")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--ctx", type=int, default=2048)
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--rounds", type=int, default=3, help="greedy/sampled pairs (mirrored order)")
    p.add_argument("--profile-steps", type=int, default=8)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    args = p.parse_args()

    from inferd_amd import pipeline as P
    from inferd_amd.runtime import MODELS
    d = MODELS[args.model]
    B, ctx, K, W = args.batch, args.ctx, args.steps, args.warmup
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    order = []
    for r in range(args.rounds):
        order += ["greedy", "sampled"] if r % 2 == 0 else ["sampled", "greedy"]
    per_run = W + K + args.profile_steps
    st = P.PipelineStage(d, 0, 1, 0, d.layers, device=dev, seed=args.seed, n_microbatches=1, batch=B,
                         max_ctx=ctx + len(order) * per_run + 2 * args.profile_steps + 64, prefill_chunk=2)
    g = torch.Generator().manual_seed(args.seed + 17)
    st.prefill([torch.randint(0, d.vocab, (B, ctx), generator=g)])
    torch.cuda.synchronize()
    span = st.span
    runs = []
    for i, mode in enumerate(order):
        if mode == "sampled":
            span.set_sampling(*SAMPLING, seed=args.seed)
        else:
            span.clear_sampling()
        st.prepare_decode(W + K)            # the graph bakes the head of the current setting
        st.decode(W)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st.decode(K)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / K
        prof = st.profile_decode(args.profile_steps)
        head_ms, head_n = prof["lm_head_argmax"]
        runs.append({"mode": mode, "ctx_start": ctx + i * per_run, "ms_per_step": round(ms, 4),
                     "lm_head_class_us": round(head_ms / max(head_n, 1) * 1e3, 2),
                     "kernel_sum_ms_per_step": round(sum(m for m, _ in prof.values()) / args.profile_steps, 4)})
        print(json.dumps(runs[-1]), flush=True)
        span.check_errors()
    span.clear_sampling()

    def head_us(logits):
        """the greedy head's class time over eager steps, with or without the GEMV's logits store"""
        span.profile_start(1 << 12)
        for _ in range(args.profile_steps):
            states = [span.reserve(sid, 1) for sid in st.sessions[0]]
            batch = span.build_batch([(s, 1) for s in states])
            span.run(batch, ids=st.ids[0], next_ids=st.ids[0], logits=logits)
            for s in states:
                s.length += 1
        torch.cuda.synchronize()
        ms, n = span.profile_stop()["lm_head_argmax"]
        return round(ms / max(n, 1) * 1e3, 2)
    store = {"greedy_no_logits": head_us(None),
             "greedy_logits_stored": head_us(torch.empty(B, d.vocab, dtype=torch.bfloat16, device=dev))}

    def stats(mode, key):
        v = [r[key] for r in runs if r["mode"] == mode]
        return {"mean": round(statistics.fmean(v), 4), "min": min(v), "max": max(v), "runs": v}
    gs, ss = stats("greedy", "ms_per_step"), stats("sampled", "ms_per_step")
    gh, sh = stats("greedy", "lm_head_class_us"), stats("sampled", "lm_head_class_us")
    out = {
        "workload": f"{args.model} decode, batch {B} at {ctx} context, one span, DecodeGraph loop (next_ids feed ids)",
        "device": torch.cuda.get_device_name(dev),
        "sampling": dict(zip(("temperature", "top_k", "top_p"), SAMPLING)),
        "steps": K, "warmup": W, "rounds": args.rounds, "order": order,
        "ms_per_step": {"greedy": gs, "sampled": ss},
        "sampled_minus_greedy_us": round((ss["mean"] - gs["mean"]) * 1e3, 2),
        "run_to_run_spread_us": {"greedy": round((gs["max"] - gs["min"]) * 1e3, 2),
                                 "sampled": round((ss["max"] - ss["min"]) * 1e3, 2)},
        "lm_head_class_us": {"greedy": gh, "sampled": sh,
                             "sampled_minus_greedy": round(sh["mean"] - gh["mean"], 2),
                             # the two parts of that difference: the logits store inside the GEMV launch (a
                             # greedy head that also stores them), and the sampling kernel in place of argmax_reduce
                             **store,
                             "logits_store": round(store["greedy_logits_stored"] - store["greedy_no_logits"], 2),
                             "sampling_kernel_minus_argmax_reduce":
                                 round(sh["mean"] - gh["mean"] - store["greedy_logits_stored"]
                                       + store["greedy_no_logits"], 2)},
        "runs": runs,
        "note": "ms_per_step: K steps between two events on the launch stream (includes the host's launch pace); "
                "lm_head_class_us: eager event pairs around final norm + lm_head GEMV + argmax reduce / sampling "
                "kernel; the context grows by warmup + steps + profile steps per run, the mirrored order cancels it "
                "in the means",
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("ms_per_step", "sampled_minus_greedy_us", "run_to_run_spread_us",
                                          "lm_head_class_us")}))


if __name__ == "__main__":
    main()
