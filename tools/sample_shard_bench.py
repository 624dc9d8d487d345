#!/usr/bin/env python3
"""What one stage's shard of a SAMPLED vocab-parallel head costs over the greedy shard, at Qwen3-8B
head geometry (hidden 4096, B = 16, a shard of 18,992 lm_head rows = vocab / 8), beside the whole-head
sampling kernel at vocab 151,936 in the same run.

Calls timed (temperature 0.6, top-k 20, top-p 0.95; normed rows random, weights synthetic):
    greedy            inferd_span_head_shard, keys_in -> keys_out          (GEMV + argmax_keys)
    greedy_logits     the same with the shard's logits stored              (the GEMV's extra store)
    sampled_mid       inferd_span_head_shard_sampled, cand_in -> cand_out  (GEMV + shard kernel)
    sampled_finish    the same with cand_in -> ids                         (GEMV + shard kernel + draw)
    whole_sample_op   inferd_sample on bf16 logits [16, 151936]            (the whole-head kernel alone,
                      tile maxima from the logits)
    shard_sample_op   inferd_sample_shard on [16, 18992] with cand_in      (the shard kernel alone, likewise)
    whole_greedy / whole_sampled   a whole-head span through the same two entry points (all 151,936 rows)
Two figures per call: `loop_us` = N launches back to back between two HIP events on the stream, after
W warm-up launches (includes the host's launch pace when that is the slower side), and, for span
calls, `class_us` = the engine's own event pair around the call's launches (INFERD_PROF_LMHEAD).
Each figure is the median of `--rounds` repetitions; min and max are kept.

    python tools/sample_shard_bench.py [--launches 200] [--warmup 20] [--rounds 5] [--out profiles/sample_shard_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLING = (0.6, 20, 0.95, 1234)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="qwen3-8b")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--parts", type=int, default=8)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_shard_bench.json"))
    args = p.parse_args()

    from inferd_amd import runtime as RT
    d = RT.MODELS[args.model]
    B, N, W = args.batch, args.launches, args.warmup
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = d.vocab // args.parts // 16 * 16
    first = rows                                   # the second shard: an earlier one has filled the record

    def span(**kw):
        s = RT.SpanRuntime(d, 0, 0, has_embed=False, device=dev, kv_pages=16, max_tokens=64, max_seqs=B,
                           max_positions=64, **kw)
        s.init_synthetic(1234)
        return s
    shard = span(has_lm_head=False, head_first=first, head_rows=rows)
    whole = span(has_lm_head=True)
    g = torch.Generator().manual_seed(5)
    from inferd_amd.pipeline import pack_rows
    nt = torch.zeros(shard.normed_elems(B), dtype=torch.bfloat16, device=dev)
    packed = pack_rows((torch.randn(B, d.hidden, generator=g) * 0.7).to(torch.bfloat16).to(dev))
    nt[:packed.numel()].copy_(packed)
    rs = RT.row_seed_tensor(list(range(B)), dev)
    pos = torch.full((B,), 2048, dtype=torch.int32, device=dev)
    ids = torch.zeros(B, dtype=torch.int32, device=dev)
    keys_in = torch.zeros(B, dtype=torch.int64, device=dev)
    keys_out = torch.zeros(B, dtype=torch.int64, device=dev)
    lg_shard = torch.empty(B, rows, dtype=torch.bfloat16, device=dev)
    lg_whole = torch.empty(B, d.vocab, dtype=torch.bfloat16, device=dev)
    # a realistic record of the shard before: the first shard's columns of the whole head's logits
    whole.head_shard(nt, B, ids=ids, logits=lg_whole)
    cand_in = RT.cand_record(B, dev)
    RT.sample_shard(lg_whole[:, :first].contiguous(), 0, *SAMPLING, cand_out=cand_in, row_seeds=rs)
    cand_out = RT.cand_record(B, dev)
    lg_mid = lg_whole[:, first:first + rows].contiguous()
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    T = torch.ops.inferd
    t, k, pp, seed = SAMPLING

    calls = {
        "greedy": (shard, lambda: shard.head_shard(nt, B, keys_in=keys_in, keys_out=keys_out)),
        "greedy_logits": (shard, lambda: shard.head_shard(nt, B, keys_in=keys_in, keys_out=keys_out, logits=lg_shard)),
        "sampled_mid": (shard, lambda: shard.head_shard_sampled(nt, B, SAMPLING, rs, cand_in=cand_in, cand_out=cand_out)),
        "sampled_finish": (shard, lambda: shard.head_shard_sampled(nt, B, SAMPLING, rs, cand_in=cand_in, positions=pos,
                                                                   ids=ids)),
        "whole_sample_op": (None, lambda: T.sample(lg_whole, t, k, pp, seed, rs, pos, ids, None, flags)),
        "shard_sample_op": (None, lambda: T.sample_shard(lg_mid, B, first, t, k, pp, seed, rs, cand_in, cand_out, None,
                                                         None, None, flags)),
        "whole_greedy": (whole, lambda: whole.head_shard(nt, B, ids=ids, logits=lg_whole)),
        "whole_sampled": (whole, lambda: whole.head_shard_sampled(nt, B, SAMPLING, rs, positions=pos, ids=ids,
                                                                  logits=lg_whole)),
    }

    def loop_us(fn):
        for _ in range(W):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / N * 1e3

    def class_us(sp, fn):
        sp.profile_start(4 * N)
        for _ in range(N):
            fn()
        torch.cuda.synchronize()
        ms, n = sp.profile_stop()["lm_head_argmax"]
        return ms / max(n, 1) * 1e3

    def summary(v):
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    res = {name: {"loop_us": [], "class_us": []} for name in calls}
    for _ in range(args.rounds):                  # the calls interleaved: drift hits all of them alike
        for name, (sp, fn) in calls.items():
            res[name]["loop_us"].append(loop_us(fn))
            if sp is not None:
                res[name]["class_us"].append(class_us(sp, fn))
    for sp in (shard, whole):
        sp.check_errors()
    out = {"workload": f"{args.model} head geometry: hidden {d.hidden}, batch {B}, shard rows {rows} of vocab {d.vocab}",
           "device": torch.cuda.get_device_name(dev),
           "sampling": dict(zip(("temperature", "top_k", "top_p"), SAMPLING[:3])),
           "launches": N, "warmup": W, "rounds": args.rounds,
           "record_bytes_per_hop": {"sampled": B * RT.SAMPLE_CAND_WORDS * 8, "greedy": B * 8},
           "calls": {name: {key: summary(v) for key, v in r.items() if v} for name, r in res.items()}}
    c = out["calls"]
    pick = "class_us"
    out["derived_us"] = {
        "basis": pick,
        "sampled_mid_minus_greedy": round(c["sampled_mid"][pick]["median"] - c["greedy"][pick]["median"], 2),
        "sampled_finish_minus_greedy": round(c["sampled_finish"][pick]["median"] - c["greedy"][pick]["median"], 2),
        "of_which_logits_store": round(c["greedy_logits"][pick]["median"] - c["greedy"][pick]["median"], 2),
        "whole_sample_kernel_alone_loop": c["whole_sample_op"]["loop_us"]["median"],
        "shard_sample_kernel_alone_loop": c["shard_sample_op"]["loop_us"]["median"],
        "whole_sampled_minus_whole_greedy": round(c["whole_sampled"][pick]["median"] - c["whole_greedy"][pick]["median"], 2)}
    out["note"] = ("loop_us: N launches between two events after warm-up (host launch pace included); class_us: the "
                   "engine's event pair around each call's launches; medians of the rounds.  The record's cost on a "
                   "real xGMI hop is not measured here: no multi-GPU RCCL run of the sampled ring exists yet.")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"calls": {n: {k2: v["median"] for k2, v in r.items()} for n, r in c.items()},
                      "derived_us": out["derived_us"]}))


if __name__ == "__main__":
    main()
