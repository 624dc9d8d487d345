"""Span-level parity of the HIP path against the oracle and the reference's golden vectors.

Tolerance (stated once, used everywhere below): a bf16 hidden state H_gpu matches the
reference H_ref when  max|H_gpu - H_ref| <= TOL_REL * max|H_ref|  (per tensor), with
TOL_REL = 2e-2 against the oracle run with the same attention semantics (sdpa) and
3e-2 against the gRPC golden (eager attention rounds scores to bf16, the kernel keeps
them in fp32).  Greedy tokens are checked on the "peaked" synthetic profile (large top-1
margins, oracle/weightgen.py) on EVERY step, and every step's reference margin must exceed
twice the measured logit error, so agreement is never luck and never skipped.
"""
import os
import subprocess

import pytest
import torch

from golden_io import load, tensor
from oracle import qwen3_ref as R

pytestmark = pytest.mark.gpu

SEED = 1234
DEV = "cuda"
TOL_REL = 2e-2
TOL_REL_EAGER = 3e-2


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def span(cfg, first, n, embed, lm, profile="random", **kw):
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS[cfg]
    s = SpanRuntime(d, first, n, has_embed=embed, has_lm_head=lm, device=DEV,
                    max_positions=kw.pop("max_positions", 8192), **kw)
    s.init_synthetic(SEED, profile)
    return s


def max_abs(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().max().item()


def test_tiny_two_spans_vs_golden():
    g = load("tiny_petals.npz")
    prompt = torch.from_numpy(g["prompt"])
    s0 = span("tiny", 0, 2, True, False)
    s1 = span("tiny", 2, 2, False, True)
    o0 = s0.forward([(None, 16)], ids=prompt, want_layers=True)
    o1 = s1.forward([(None, 16)], x=o0["hidden"], want_layers=True, want_next_ids=True, want_logits=True)
    layers = torch.cat([o0["layers"], o1["layers"]], 0)
    for i in range(4):
        e = rel_err(layers[i], tensor(g[f"bf16_layer{i}"])[0])
        print(f"tiny layer {i}: rel err {e:.2e}")
        assert e < TOL_REL, (i, e)
    lg = tensor(g["bf16_logits"])[0, -1]
    e = rel_err(o1["logits"][0], lg)
    print(f"tiny last-row logits rel err {e:.2e}")
    assert e < TOL_REL


def test_tiny_two_spans_free_running_vs_reference_chain():
    """The reference's OWN chain (tiny_petals_peaked.npz: the real PartitionedQwen2.forward
    chain and its bf16 stage modules, peaked profile, 16 free-running greedy steps of full
    recompute, send_message.py:46-60) against two HIP spans free-running the same protocol:
    all 16 ids identical, and at every step the reference chain's margin exceeds twice the
    engine's measured logit error (against the oracle on the same prefix)."""
    g = load("tiny_petals_peaked.npz")
    ref_ids = g["bf16_greedy_ids"].tolist()
    assert ref_ids == g["fp32_greedy_ids"].tolist()      # the reference chain agrees with itself
    s0 = span("tiny", 0, 2, True, False, "peaked")
    s1 = span("tiny", 2, 2, False, True, "peaked")
    b0 = R.RefSpan(R.CONFIGS["tiny"], SEED, 0, 1, True, False, profile="peaked")
    b1 = R.RefSpan(R.CONFIGS["tiny"], SEED, 2, 3, False, True, profile="peaked")
    ids = g["prompt"].tolist()
    for step, (rid, margin) in enumerate(zip(ref_ids, g["bf16_margins"].tolist())):
        x = torch.tensor(ids)
        h = s0.forward([(None, len(ids))], ids=x)["hidden"]
        o = s1.forward([(None, len(ids))], x=h, want_next_ids=True, want_logits=True, want_hidden=False)
        nid = int(o["next_ids"][0])
        err = max_abs(o["logits"][0], b1.forward(b0.forward(x[None]))[0, -1])
        print(f"step {step}: gpu {nid} ref {rid} margin {margin:.3f} logit err {err:.3e}")
        assert nid == rid, step
        assert margin > 2 * err, (step, margin, err)
        ids.append(nid)  # free-running: the GPU chain feeds back its own ids


def test_q06_layer_cached_vs_golden():
    g = load("q06_layer.npz")
    s = span("qwen3-0.6b", int(g["start"]), 1, False, False)
    oracle = R.RefSpan(R.CONFIGS["qwen3-0.6b"], SEED, int(g["start"]), int(g["end"]), False, False,
                       torch.bfloat16, "sdpa")
    ins = [tensor(g["bf16_in_prefill"])] + [tensor(g[f"bf16_in_dec{i}"]) for i in range(4)]
    for i, x in enumerate(ins):
        T = x.shape[1]
        out = s.forward([("sess", T)], x=x[0])["hidden"]
        ref_o = oracle.forward_cached("sess", x)[0]
        e_or = rel_err(out, ref_o)
        e_gold = rel_err(out, tensor(g[f"bf16_out{i}"])[0])
        print(f"q06 call {i}: vs oracle(sdpa) {e_or:.2e}  vs golden(eager) {e_gold:.2e}")
        assert e_or < TOL_REL and e_gold < TOL_REL_EAGER


def test_q8b_layer_batched_cached_vs_golden():
    g = load("q8b_layer.npz")
    s = span("qwen3-8b", int(g["start"]), 1, False, False, max_tokens=64)
    ins = [tensor(g["bf16_in_prefill"])] + [tensor(g[f"bf16_in_dec{i}"]) for i in range(2)]
    for i, x in enumerate(ins):
        B, T = x.shape[0], x.shape[1]
        out = s.forward([(f"s{b}", T) for b in range(B)], x=x.reshape(B * T, -1))["hidden"]
        e = rel_err(out, tensor(g[f"bf16_out{i}"]).reshape(B * T, -1))
        print(f"q8b call {i}: vs golden(eager) {e:.2e}")
        assert e < TOL_REL_EAGER


def test_partitioned_qwen2_dict_protocol(tmp_path):
    """The node-facing API end to end: stage files written by the offline splitter, two
    PartitionedQwen2 stages chained through the reference's dict protocol (generated_ids ->
    hidden_meta (bf16 wire codec) -> next_token_id), 16 free-running greedy steps of full
    recompute as in send_message.py:46-60, against EVERY id of the reference's own chain
    (tiny_petals_peaked.npz, peaked profile)."""
    from inferd_amd.partitioned_models import PartitionedQwen2
    from inferd_amd.runtime import MODELS
    from inferd_amd.split_model import split
    g = load("tiny_petals_peaked.npz")
    d = R.CONFIGS["tiny"]
    cfg = {"model_name": "tiny", "parts_dir": str(tmp_path), "stages_count": 2,
           "stages": [{"name": "node0", "stage": 0, "start_layer": 0, "end_layer": 1},
                      {"name": "node1", "stage": 1, "start_layer": 2, "end_layer": 3}]}
    glob = R.gen_global_weights(d, SEED, profile="peaked")
    attn = ("q_proj", "k_proj", "v_proj", "o_proj", "q_norm", "k_norm")

    def get_layer(i):
        return {("self_attn." if k in attn else "mlp." if k.endswith("_proj") else "") + k + ".weight": v
                for k, v in R.gen_layer_weights(d, SEED, i).items()}
    p0, p1 = split(cfg, MODELS["tiny"], get_layer, lambda n: glob[n])
    n0 = PartitionedQwen2("tiny", 2, 0, p0)
    n1 = PartitionedQwen2("tiny", 2, 1, p1)
    ids = g["prompt"].tolist()
    ref_ids = g["fp32_greedy_ids"].tolist()   # the real PartitionedQwen2.forward chain's
    for step in range(len(ref_ids)):
        o0 = n0.forward({"generated_ids": ids})
        assert o0["hidden_meta"]["dtype"] == "bfloat16" and o0["generated_ids"] == ids
        o1 = n1.forward(o0)
        assert o1["next_token_id"] == ref_ids[step], step
        assert o1["generated_ids"] == ids + [o1["next_token_id"]]
        ids = o1["generated_ids"]                 # free-running
    # synthetic stage spec gives the same model without files
    s0 = PartitionedQwen2("tiny", 2, 0, f"synthetic:{SEED}:tiny:0:1:peaked")
    h_file = n0.forward({"generated_ids": ids})["hidden_meta"]
    h_syn = s0.forward({"generated_ids": ids})["hidden_meta"]
    assert h_file == h_syn


def test_decode_graph_matches_eager():
    """A captured decode step (device-side position advance + whole span) replayed n times
    gives bit-identical ids/logit-argmax to n eager cached decode calls."""
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["tiny"]
    prompts = torch.randint(0, d.vocab, (3, 70), generator=torch.Generator().manual_seed(9))
    runs = []
    for use_graph in (False, True):
        s = span("tiny", 0, d.layers, True, True)
        sess = [f"g{b}" for b in range(3)]
        out = s.forward([(sid, 70) for sid in sess], ids=prompts.reshape(-1), want_next_ids=True, want_hidden=False)
        ids = out["next_ids"].clone()
        seq = [ids.cpu().clone()]
        if use_graph:
            g = DecodeGraph(s, sess, 6, ids=ids, next_ids=ids)
            for _ in range(6):
                g.launch()
                seq.append(ids.cpu().clone())
        else:
            for _ in range(6):
                ids = s.forward([(sid, 1) for sid in sess], ids=ids, want_next_ids=True, want_hidden=False)["next_ids"]
                seq.append(ids.cpu().clone())
        runs.append(torch.stack(seq))
    assert torch.equal(runs[0], runs[1]), (runs[0], runs[1])


@pytest.mark.parametrize("first", [True, False])
def test_decode_graph_hidden_bit_exact(first):
    """The decode graph's first launch carries the scheduler step and (first span) the
    embedding gather inside layer 0's input norm (span.hip NormPrologue); an eager cached
    decode call launches the same kernels without the step.  Both give bit-identical hidden
    states over 4 steps, for a first span (ids in) and an inner span (x in)."""
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["tiny"]
    gen = torch.Generator().manual_seed(21)
    prompts = torch.randint(0, d.vocab, (3, 40), generator=gen)
    steps_ids = torch.randint(0, d.vocab, (4, 3), generator=gen)
    x_pre = (torch.randn(3 * 40, d.hidden, generator=gen) * 0.5).to(torch.bfloat16)
    x_steps = (torch.randn(4, 3, d.hidden, generator=gen) * 0.5).to(torch.bfloat16)
    runs = []
    for use_graph in (False, True):
        s = span("tiny", 0 if first else 1, 2, first, False)
        sess = [f"h{b}" for b in range(3)]
        if first:
            s.forward([(sid, 40) for sid in sess], ids=prompts.reshape(-1), want_hidden=False)
        else:
            s.forward([(sid, 40) for sid in sess], x=x_pre, want_hidden=False)
        ids = torch.zeros(3, dtype=torch.int32, device=DEV)
        xin = torch.zeros(3, d.hidden, dtype=torch.bfloat16, device=DEV)
        hout = torch.zeros(3, d.hidden, dtype=torch.bfloat16, device=DEV)
        g = None
        if use_graph:
            g = DecodeGraph(s, sess, 4, ids=ids if first else None, x=None if first else xin, hidden_out=hout)
        seq = []
        for k in range(4):
            ids.copy_(steps_ids[k])
            xin.copy_(x_steps[k])
            if use_graph:
                g.launch()
                seq.append(hout.cpu().clone())
            else:
                kw = {"ids": ids} if first else {"x": xin}
                seq.append(s.forward([(sid, 1) for sid in sess], **kw)["hidden"].cpu().clone())
        runs.append(torch.stack(seq))
    assert torch.equal(runs[0], runs[1]), (runs[0] - runs[1]).abs().max()


@pytest.mark.parametrize("T,eager", [(70, False), ((70, 9, 33), True)], ids=["graph", "ragged_eager"])
def test_half_layer_stage_chain_bit_exact(T, eager):
    """Sub-layer stage boundaries (InferdSpanConfig skip_first_attn / skip_last_mlp): Qwen3-0.6B
    layers 0..3 as three spans cut between a layer's attention and MLP halves -- [0..1a] (embed),
    [1m..2a], [2m..3] (lm_head) -- give bit-identical logits to one span over the same layers,
    for a 70-token prefill of 3 sequences and 5 decode-graph steps (teacher-forced, the chain's
    graphs replayed in stage order on fixed hand-off buffers); the first boundary's hidden state
    (layer 1's post-attention residual h1) is within the span tolerance of the oracle's.
    "ragged_eager": ragged prompts, and the chain's decode steps launched kernel by kernel
    (`inferd_span_step`, the pipeline's default) against the single span's graph replays."""
    from inferd_amd.pipeline import StageRange
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["qwen3-0.6b"]
    B, STEPS = 3, 5
    gen = torch.Generator().manual_seed(31)
    lens = T if isinstance(T, tuple) else (T,) * B
    prompts = [torch.randint(0, d.vocab, (n,), generator=gen) for n in lens]
    ids = torch.cat(prompts)
    forced = torch.randint(0, d.vocab, (STEPS, B), generator=gen)
    ranges = [StageRange(0, 3), StageRange(3, 2), StageRange(5, 3)]
    chain = [span("qwen3-0.6b", r.first_layer, r.n_layers, i == 0, i == 2, kv_pages=16, max_tokens=len(ids),
                  max_seqs=B, max_positions=1024, skip_first_attn=r.skip_first_attn, skip_last_mlp=r.skip_last_mlp)
             for i, r in enumerate(ranges)]
    one = span("qwen3-0.6b", 0, 4, True, True, kv_pages=16, max_tokens=len(ids), max_seqs=B, max_positions=1024)
    sess = [f"c{b}" for b in range(B)]
    reqs = [(sid, n) for sid, n in zip(sess, lens)]
    h0 = chain[0].forward(reqs, ids=ids)["hidden"]
    h1 = chain[1].forward(reqs, x=h0)["hidden"]
    lc = chain[2].forward(reqs, x=h1, want_logits=True, want_hidden=False)["logits"]
    lo = one.forward(reqs, ids=ids, want_logits=True, want_hidden=False)["logits"]
    assert torch.equal(lc, lo), (lc.float() - lo.float()).abs().max()
    ref = R.RefSpan(d, SEED, 0, 1, True, False, skip_last_mlp=True)
    hv = h0.reshape(len(ids), -1)
    e, off = 0.0, 0
    for p in prompts:   # per sequence (ragged prompts: each its own oracle forward)
        e = max(e, rel_err(hv[off:off + len(p)].view(1, len(p), -1), ref.forward(p.view(1, -1))))
        off += len(p)
    print(f"half-layer boundary (layer 1's h1) vs oracle: rel err {e:.2e}")
    assert e < TOL_REL
    ids_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    ids_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    hb = [torch.zeros(B, d.hidden, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    lg_c = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    lg_o = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    nid_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    nid_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    graphs = [DecodeGraph(chain[0], sess, STEPS, ids=ids_c, hidden_out=hb[0]),
              DecodeGraph(chain[1], sess, STEPS, x=hb[0], hidden_out=hb[1]),
              DecodeGraph(chain[2], sess, STEPS, x=hb[1], next_ids=nid_c, logits=lg_c)]
    g1 = DecodeGraph(one, sess, STEPS, ids=ids_o, next_ids=nid_o, logits=lg_o)
    for k in range(STEPS):
        ids_c.copy_(forced[k])
        ids_o.copy_(forced[k])
        for g in graphs:
            g.launch_eager() if eager else g.launch()
        g1.launch()
        assert torch.equal(lg_c, lg_o), (k, (lg_c.float() - lg_o.float()).abs().max())
        assert torch.equal(nid_c, nid_o), k
    for s in chain + [one]:
        s.check_errors()


@pytest.mark.parametrize("T", [70, 9, (70, 9, 33), (30, 9, 17)],
                         ids=["prefill_h1", "prefill_record", "ragged_h1", "ragged_record"])
def test_gateup_boundary_chain_bit_exact(T):
    """Stage boundaries inside a layer's gate/up projection (InferdSpanConfig gateup_split_*):
    Qwen3-0.6B layers 0..3 as [0..1a+1024] (embed), [1m@1024..2a+2048], [2m@2048..3] (lm_head)
    give bit-identical logits to one span: a prefill of 3 sequences (T = 70: 210 rows, h1
    hand-offs, the receiver runs the whole MLP; T = 9: 27 rows, decode-sized calls with record
    hand-offs), then 5 decode-graph steps whose hand-offs are records (h1, then act columns
    [0, c) fragment-packed, completed in place by the receiver).  A tuple T gives ragged prompts
    (112 rows: h1 hand-offs; 56 rows: records)."""
    from inferd_amd.pipeline import StageRange, handoff_elems, record_elems
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["qwen3-0.6b"]
    B, STEPS = 3, 5
    gen = torch.Generator().manual_seed(41)
    lens = T if isinstance(T, tuple) else (T,) * B
    ids = torch.randint(0, d.vocab, (sum(lens),), generator=gen)
    forced = torch.randint(0, d.vocab, (STEPS, B), generator=gen)
    ranges = [StageRange(0, 3, 0, 1024), StageRange(3, 2, 1024, 2048), StageRange(5, 3, 2048, 0)]
    chain = [span("qwen3-0.6b", r.first_layer, r.n_layers, i == 0, i == 2, kv_pages=16, max_tokens=sum(lens) + 64,
                  max_seqs=B, max_positions=1024, **r.span_kwargs()) for i, r in enumerate(ranges)]
    one = span("qwen3-0.6b", 0, 4, True, True, kv_pages=16, max_tokens=sum(lens) + 64, max_seqs=B,
               max_positions=1024)
    sess = [f"g{b}" for b in range(B)]
    reqs = [(sid, n) for sid, n in zip(sess, lens)]
    o0 = chain[0].forward(reqs, ids=ids)
    h0 = o0.get("record", o0["hidden"])
    o1 = chain[1].forward(reqs, x=h0)
    h1 = o1.get("record", o1["hidden"])
    assert ("record" in o0) == (sum(lens) <= 64)
    lc = chain[2].forward(reqs, x=h1, want_logits=True, want_hidden=False)["logits"]
    lo = one.forward(reqs, ids=ids, want_logits=True, want_hidden=False)["logits"]
    assert torch.equal(lc, lo), (lc.float() - lo.float()).abs().max()
    ids_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    ids_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    recs = [torch.zeros(record_elems(d, B), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    lg_c = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    lg_o = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    nid_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    nid_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    graphs = [DecodeGraph(chain[0], sess, STEPS, ids=ids_c, hidden_out=recs[0]),
              DecodeGraph(chain[1], sess, STEPS, x=recs[0], hidden_out=recs[1]),
              DecodeGraph(chain[2], sess, STEPS, x=recs[1], next_ids=nid_c, logits=lg_c)]
    g1 = DecodeGraph(one, sess, STEPS, ids=ids_o, next_ids=nid_o, logits=lg_o)
    assert handoff_elems(d, B, 1024) == B * d.hidden + 16 * 1024
    for k in range(STEPS):
        ids_c.copy_(forced[k])
        ids_o.copy_(forced[k])
        for g in graphs:
            g.launch()
        g1.launch()
        assert torch.equal(lg_c, lg_o), (k, (lg_c.float() - lg_o.float()).abs().max())
        assert torch.equal(nid_c, nid_o), k
    for s in chain + [one]:
        s.check_errors()


@pytest.mark.parametrize("split,T", [("o", 70), ("o", 9), ("o_gateup", 9), ("q", 70), ("q", 9), ("q_o", 9),
                                     ("o", (70, 9, 33)), ("q_o", (70, 9, 33))],
                         ids=["o_prefill_rows", "o_prefill_small", "o_then_gateup", "q_prefill_rows", "q_prefill_small",
                              "q_then_o", "o_ragged", "q_then_o_ragged"])
def test_o_boundary_chain_bit_exact(split, T):
    """Stage boundaries between a layer's attention and its o projection (InferdSpanConfig
    o_split_*): Qwen3-0.6B layers 0..3 as [0..1q] (embed), [1o..3q], [3o..3] (lm_head) -- or
    [0..1q], [1o..2a+1024], [2m@1024..3] (an attention|o boundary and a gate/up one) -- give
    bit-identical logits to one span: a prefill of 3 sequences (the record x | attention output
    row-major), then 5 decode-graph steps whose records carry the attention output fragment-packed.
    The first record's attention output (layer 1's, before o_proj) is within the span tolerance of
    the oracle's.  "q" / "q_o": q/k/v|attention boundaries (InferdSpanConfig qkv_split_*) in
    place of the first (and second) ones -- prefill hands over x alone and the receiver runs the
    whole layer; decode records carry x and the raw q/k/v rows (split-K slices summed by the
    sender as the fused attention sums them).  A tuple T gives ragged prompts (one length per sequence):
    the prefill record's rows and every decode step's contexts then differ per sequence."""
    from inferd_amd.pipeline import StageRange, buffer_elems, o_record_elems, unpack_rows
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["qwen3-0.6b"]
    B, STEPS = 3, 5
    Hd = d.heads * d.head_dim
    gen = torch.Generator().manual_seed(43)
    lens = T if isinstance(T, tuple) else (T,) * B
    prompts = [torch.randint(0, d.vocab, (n,), generator=gen) for n in lens]
    forced = torch.randint(0, d.vocab, (STEPS, B), generator=gen)
    N = sum(lens)
    if split == "o":
        ranges = [StageRange(0, 3, last_o=True), StageRange(2, 5, first_o=True, last_o=True),
                  StageRange(6, 2, first_o=True)]
    elif split == "q":
        ranges = [StageRange(0, 3, last_q=True), StageRange(2, 5, first_q=True, last_q=True),
                  StageRange(6, 2, first_q=True)]
    elif split == "q_o":
        ranges = [StageRange(0, 3, last_q=True), StageRange(2, 5, first_q=True, last_o=True),
                  StageRange(6, 2, first_o=True)]
    else:
        ranges = [StageRange(0, 3, last_o=True), StageRange(2, 3, 0, 1024, first_o=True), StageRange(5, 3, 1024, 0)]
    chain = [span("qwen3-0.6b", r.first_layer, r.n_layers, i == 0, i == 2, kv_pages=16, max_tokens=N + 64,
                  max_seqs=B, max_positions=1024, **r.span_kwargs()) for i, r in enumerate(ranges)]
    one = span("qwen3-0.6b", 0, 4, True, True, kv_pages=16, max_tokens=N + 64, max_seqs=B, max_positions=1024)
    sess = [f"o{b}" for b in range(B)]
    reqs = [(sid, n) for sid, n in zip(sess, lens)]
    ids = torch.cat(prompts)
    o0 = chain[0].forward(reqs, ids=ids)
    qsplit = split.startswith("q")
    rec0 = o0["hidden"].reshape(-1) if qsplit else o0["record"]
    assert rec0.numel() == (N * d.hidden if qsplit else o_record_elems(d, N, False))
    o1 = chain[1].forward(reqs, x=rec0)
    lc = chain[2].forward(reqs, x=o1.get("record", o1["hidden"]), want_logits=True, want_hidden=False)["logits"]
    lo = one.forward(reqs, ids=ids, want_logits=True, want_hidden=False)["logits"]
    assert torch.equal(lc, lo), (lc.float() - lo.float()).abs().max()
    ref = R.RefSpan(d, SEED, 0, 1, True, False, o_split_last=not qsplit, qkv_split_last=qsplit)
    xa = rec0[:N * d.hidden].view(N, -1)
    aa = None if qsplit else rec0[N * d.hidden:].view(N, -1)
    ex = ea = 0.0
    off = 0
    for p in prompts:   # per sequence (ragged prompts: each its own oracle forward)
        xr, ar = ref.forward(p.view(1, -1))
        ex = max(ex, rel_err(xa[off:off + len(p)].view(1, len(p), -1), xr))
        if aa is not None:
            ea = max(ea, rel_err(aa[off:off + len(p)].view(1, len(p), -1), ar))
        off += len(p)
    print(f"{split} record vs oracle: x rel err {ex:.2e}, attention output rel err {ea:.2e}")
    assert ex < TOL_REL and ea < TOL_REL
    ids_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    ids_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    r0, r1 = ranges[0], ranges[1]
    recs = [torch.zeros(buffer_elems(d, B, r.last_col, r.last_o, True, r.last_q), dtype=torch.bfloat16, device=DEV)
            for r in (r0, r1)]
    lg_c = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    lg_o = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    nid_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    nid_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    graphs = [DecodeGraph(chain[0], sess, STEPS, ids=ids_c, hidden_out=recs[0]),
              DecodeGraph(chain[1], sess, STEPS, x=recs[0], hidden_out=recs[1]),
              DecodeGraph(chain[2], sess, STEPS, x=recs[1], next_ids=nid_c, logits=lg_c)]
    g1 = DecodeGraph(one, sess, STEPS, ids=ids_o, next_ids=nid_o, logits=lg_o)
    Nq = (d.heads + 2 * d.kv_heads) * d.head_dim
    assert recs[0].numel() == B * d.hidden + (B * Nq if qsplit else 16 * Hd)
    for k in range(STEPS):
        ids_c.copy_(forced[k])
        ids_o.copy_(forced[k])
        for g in graphs:
            g.launch()
        g1.launch()
        assert torch.equal(lg_c, lg_o), (k, (lg_c.float() - lg_o.float()).abs().max())
        assert torch.equal(nid_c, nid_o), k
    if qsplit:   # the decode record's q/k/v rows: the oracle's projection of the record's x
        xq = recs[0][:B * d.hidden].view(B, 1, d.hidden).cpu()
        qr = R.qkv_proj(xq, R.RefSpan(d, SEED, 1, 1, False, False).layers[0], d)
        eq = rel_err(recs[0][B * d.hidden:].view(B, 1, Nq), qr)
        print(f"q/k/v record rows vs oracle: rel err {eq:.2e}")
        assert eq < TOL_REL
    else:        # the decode record's attention output is fragment-packed: its padding rows stay zero
        a = unpack_rows(recs[0][B * d.hidden:], 16, Hd)
        assert torch.count_nonzero(a[B:]) == 0 and torch.count_nonzero(a[:B]) > 0
    for s in chain + [one]:
        s.check_errors()


@pytest.mark.parametrize("T", [9, (30, 9, 17)], ids=["prefill_small", "ragged"])
@pytest.mark.parametrize("split,first", [("o", False), ("q", False), ("q", True), ("o", True)],
                         ids=["o_middle", "q_middle", "q_first", "o_first"])
def test_one_layer_record_span_chain_bit_exact(split, first, T):
    """One-layer spans that end at a record boundary: the record's first part is the span's own
    input, copied there -- the caller's x_in ("middle": Qwen3-0.6B layers 0..3 as [0], [1..1q] or
    [1..1v], [1o..3] or [1k..3] with lm_head) or the span's embedding output ("first": [0..0q] or
    [0..0v] with the embedding, [0o..1] or [0k..1], [2..3]).  Each chain gives bit-identical logits and ids to one
    span over the four layers, at the prefill of 3 sequences and at each of 5 decode-graph steps
    with forced ids."""
    from inferd_amd.pipeline import StageRange, buffer_elems
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["qwen3-0.6b"]
    B, STEPS = 3, 5
    gen = torch.Generator().manual_seed(47)
    lens = T if isinstance(T, tuple) else (T,) * B
    N = sum(lens)
    ids = torch.randint(0, d.vocab, (N,), generator=gen)
    forced = torch.randint(0, d.vocab, (STEPS, B), generator=gen)
    o, q = split == "o", split == "q"
    if first:
        ranges = [StageRange(0, 1, last_o=o, last_q=q), StageRange(0, 4, first_o=o, first_q=q), StageRange(4, 4)]
    else:
        ranges = [StageRange(0, 2), StageRange(2, 1, last_o=o, last_q=q), StageRange(2, 6, first_o=o, first_q=q)]
    assert ranges[0 if first else 1].n_layers == 1
    chain = [span("qwen3-0.6b", r.first_layer, r.n_layers, i == 0, i == 2, kv_pages=16, max_tokens=N + 64,
                  max_seqs=B, max_positions=1024, **r.span_kwargs()) for i, r in enumerate(ranges)]
    one = span("qwen3-0.6b", 0, 4, True, True, kv_pages=16, max_tokens=N + 64, max_seqs=B, max_positions=1024)
    sess = [f"r{b}" for b in range(B)]
    reqs = [(sid, n) for sid, n in zip(sess, lens)]
    o0 = chain[0].forward(reqs, ids=ids)
    o1 = chain[1].forward(reqs, x=o0.get("record", o0["hidden"]))
    oc = chain[2].forward(reqs, x=o1.get("record", o1["hidden"]), want_logits=True, want_next_ids=True,
                          want_hidden=False)
    oo = one.forward(reqs, ids=ids, want_logits=True, want_next_ids=True, want_hidden=False)
    assert torch.equal(oc["logits"], oo["logits"]), (oc["logits"].float() - oo["logits"].float()).abs().max()
    assert torch.equal(oc["next_ids"], oo["next_ids"])
    ids_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    ids_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    recs = [torch.zeros(buffer_elems(d, B, r.last_col, r.last_o, True, r.last_q), dtype=torch.bfloat16, device=DEV)
            for r in ranges[:2]]
    lg_c = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    lg_o = torch.zeros(B, d.vocab, dtype=torch.bfloat16, device=DEV)
    nid_c = torch.zeros(B, dtype=torch.int32, device=DEV)
    nid_o = torch.zeros(B, dtype=torch.int32, device=DEV)
    graphs = [DecodeGraph(chain[0], sess, STEPS, ids=ids_c, hidden_out=recs[0]),
              DecodeGraph(chain[1], sess, STEPS, x=recs[0], hidden_out=recs[1]),
              DecodeGraph(chain[2], sess, STEPS, x=recs[1], next_ids=nid_c, logits=lg_c)]
    g1 = DecodeGraph(one, sess, STEPS, ids=ids_o, next_ids=nid_o, logits=lg_o)
    for k in range(STEPS):
        ids_c.copy_(forced[k])
        ids_o.copy_(forced[k])
        for g in graphs:
            g.launch()
        g1.launch()
        assert torch.equal(lg_c, lg_o), (k, (lg_c.float() - lg_o.float()).abs().max())
        assert torch.equal(nid_c, nid_o), k
    for s in chain + [one]:
        s.check_errors()


# Launches per kernel class (ops.PROF_CLASSES order: rmsnorm, q/k/v, qk-norm + rope + kv write,
# attention, o, gate/up, down, lm_head) of one forward of a 3-layer span, by span kind and call
# shape.  How to read a row: a call of <= 64 rows ("decode", "prefill9") launches one RMSNorm, the
# span's first (every later norm is folded into the GEMV that reads it), and none where the span
# starts at an o projection or at an attention; a larger call ("prefill70") launches one per norm
# the span owns.  Only a pure decode call runs qk-norm + rope inside the attention (column 3 = 0).
# A layer cut by a boundary contributes the parts on the span's side of it; a gate/up boundary's
# sender adds the gate/up prefix launch in calls of <= 64 rows; a q/k/v|attention boundary moves
# the q/k/v projection across in pure decode calls only -- other calls hand over x, so the sender's
# last layer launches nothing and the receiver runs the whole layer.
SPAN_LAUNCHES = {
    "plain": ({}, {"decode": (1, 3, 0, 3, 3, 3, 3, 1), "prefill9": (1, 3, 3, 3, 3, 3, 3, 1),
                   "prefill70": (6, 3, 3, 3, 3, 3, 3, 1)}),
    "skip_first_attn": ({"skip_first_attn": True},
                        {"decode": (1, 2, 0, 2, 2, 3, 3, 0), "prefill9": (1, 2, 2, 2, 2, 3, 3, 0),
                         "prefill70": (5, 2, 2, 2, 2, 3, 3, 0)}),
    "skip_last_mlp": ({"skip_last_mlp": True},
                      {"decode": (1, 3, 0, 3, 3, 2, 2, 0), "prefill9": (1, 3, 3, 3, 3, 2, 2, 0),
                       "prefill70": (5, 3, 3, 3, 3, 2, 2, 0)}),
    "gateup_split_first": ({"skip_first_attn": True, "gateup_split_first": 1024},
                           {"decode": (1, 2, 0, 2, 2, 3, 3, 0), "prefill9": (1, 2, 2, 2, 2, 3, 3, 0),
                            "prefill70": (5, 2, 2, 2, 2, 3, 3, 0)}),
    "gateup_split_last": ({"skip_last_mlp": True, "gateup_split_last": 1024},
                          {"decode": (1, 3, 0, 3, 3, 3, 2, 0), "prefill9": (1, 3, 3, 3, 3, 3, 2, 0),
                           "prefill70": (5, 3, 3, 3, 3, 2, 2, 0)}),
    "o_split_first": ({"o_split_first": True},
                      {"decode": (0, 2, 0, 2, 3, 3, 3, 0), "prefill9": (0, 2, 2, 2, 3, 3, 3, 0),
                       "prefill70": (5, 2, 2, 2, 3, 3, 3, 0)}),
    "o_split_last": ({"o_split_last": True},
                     {"decode": (1, 3, 0, 3, 2, 2, 2, 0), "prefill9": (1, 3, 3, 3, 2, 2, 2, 0),
                      "prefill70": (5, 3, 3, 3, 2, 2, 2, 0)}),
    "qkv_split_first": ({"qkv_split_first": True},
                        {"decode": (0, 2, 0, 3, 3, 3, 3, 0), "prefill9": (1, 3, 3, 3, 3, 3, 3, 0),
                         "prefill70": (6, 3, 3, 3, 3, 3, 3, 0)}),
    "qkv_split_last": ({"qkv_split_last": True},
                       {"decode": (1, 3, 0, 2, 2, 2, 2, 0), "prefill9": (1, 2, 2, 2, 2, 2, 2, 0),
                        "prefill70": (4, 2, 2, 2, 2, 2, 2, 0)}),
    "one_layer_o_split_last": ({"o_split_last": True, "n_layers": 1},
                               {"decode": (1, 1, 0, 1, 0, 0, 0, 0), "prefill9": (1, 1, 1, 1, 0, 0, 0, 0),
                                "prefill70": (1, 1, 1, 1, 0, 0, 0, 0)}),
}


@pytest.mark.parametrize("kind", list(SPAN_LAUNCHES))
def test_forward_launch_structure(kind):
    """The kernels one inferd_span_forward call launches, counted per class by the span's event
    profile, for every kind of span boundary at three call shapes: a 9-row prefill of 3 sequences
    (the GEMV path, not a decode batch), a pure decode call of the same 3 sequences, and a 70-row
    prefill (the tiled path).  The expected counts (SPAN_LAUNCHES) follow from the layer structure."""
    from inferd_amd.ops import PROF_CLASSES
    from inferd_amd.pipeline import buffer_elems
    kw, expected = SPAN_LAUNCHES[kind]
    kw = dict(kw)
    L = kw.pop("n_layers", 3)
    plain = kind == "plain"
    d = R.CONFIGS["qwen3-0.6b"]
    s = span("qwen3-0.6b", 0 if plain else 1, L, plain, plain, kv_pages=16, max_tokens=128, max_positions=1024, **kw)
    gen = torch.Generator().manual_seed(53)
    calls = {"prefill9": [(f"a{i}", n) for i, n in enumerate((4, 3, 2))],
             "decode": [(f"a{i}", 1) for i in range(3)],
             "prefill70": [(f"b{i}", n) for i, n in enumerate((30, 23, 17))]}
    got = {}
    for shape, reqs in calls.items():
        M = sum(n for _, n in reqs)
        pure = shape == "decode"
        if plain:
            inp = {"ids": torch.randint(0, d.vocab, (M,), generator=gen)}
        else:
            n_in = buffer_elems(d, M, s.gateup_split_first, s.o_split_first, pure, s.qkv_split_first)
            inp = {"x": (torch.randn(n_in, generator=gen) * 0.5).to(torch.bfloat16)}
        s.profile_start(256)
        s.forward(reqs, want_next_ids=plain, **inp)
        prof = s.profile_stop()
        got[shape] = tuple(prof[c][1] for c in PROF_CLASSES)
        print(f"{kind} {shape}: {got[shape]}")
    s.check_errors()
    assert got == expected


def test_half_layer_span_rejects_bad_configs():
    """A span with the embedding cannot start at a MLP half, one with lm_head cannot end at an
    attention half, a one-layer span cannot skip both halves, and a layer's absent half has no
    weights to set."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["tiny"]
    for kw in ({"has_embed": True, "has_lm_head": False, "skip_first_attn": True},
               {"has_embed": False, "has_lm_head": True, "skip_last_mlp": True}):
        with pytest.raises(RuntimeError, match="half"):
            SpanRuntime(d, 1, 2, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2, **kw)
    with pytest.raises(RuntimeError, match="both"):
        SpanRuntime(d, 1, 1, has_embed=False, has_lm_head=False, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2,
                    skip_first_attn=True, skip_last_mlp=True)
    for kw in ({"o_split_first": True, "o_split_last": True}, {"o_split_first": True, "skip_last_mlp": True}):
        with pytest.raises(RuntimeError, match="cannot end before"):
            SpanRuntime(d, 1, 1, has_embed=False, has_lm_head=False, device=DEV, kv_pages=8, max_tokens=64,
                        max_seqs=2, **kw)
    for kw in ({"has_embed": True, "o_split_first": True}, {"has_lm_head": True, "o_split_last": True},
               {"skip_first_attn": True, "o_split_first": True}):
        with pytest.raises(RuntimeError, match="attention\\|o boundary excludes"):
            SpanRuntime(d, 1, 2, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2,
                        **{"has_embed": False, "has_lm_head": False, **kw})
    for kw in ({"has_embed": True, "qkv_split_first": True}, {"has_lm_head": True, "qkv_split_last": True},
               {"o_split_first": True, "qkv_split_first": True}, {"skip_last_mlp": True, "qkv_split_last": True}):
        with pytest.raises(RuntimeError, match="attention boundary excludes"):
            SpanRuntime(d, 1, 2, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2,
                        **{"has_embed": False, "has_lm_head": False, **kw})
    with pytest.raises(RuntimeError, match="cannot end before"):
        SpanRuntime(d, 1, 1, has_embed=False, has_lm_head=False, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2,
                    qkv_split_first=True, qkv_split_last=True)
    sq = SpanRuntime(d, 1, 2, has_embed=False, has_lm_head=False, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2,
                     qkv_split_last=True)
    sq.set_weight(1, "k_proj", torch.zeros(d.kv_heads * 128, d.hidden, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="other half"):
        sq.set_weight(1, "o_proj", torch.zeros(d.hidden, d.heads * 128, dtype=torch.bfloat16))
    so = SpanRuntime(d, 1, 2, has_embed=False, has_lm_head=False, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2,
                     o_split_first=True)
    with pytest.raises(RuntimeError, match="other half"):
        so.set_weight(0, "k_proj", torch.zeros(d.kv_heads * 128, d.hidden, dtype=torch.bfloat16))
    so.set_weight(0, "o_proj", torch.zeros(d.hidden, d.heads * 128, dtype=torch.bfloat16))
    s = SpanRuntime(d, 1, 2, has_embed=False, has_lm_head=False, device=DEV, kv_pages=8, max_tokens=64, max_seqs=2,
                    skip_first_attn=True)
    with pytest.raises(RuntimeError, match="other half"):
        s.set_weight(0, "q_proj", torch.zeros(d.heads * 128, d.hidden, dtype=torch.bfloat16))
    s.set_weight(0, "down_proj", torch.zeros(d.hidden, d.intermediate, dtype=torch.bfloat16))


def test_q06_full_model_greedy_cached():
    """Config 2: Qwen3-0.6B single full span (peaked profile), prefill 32 + 12 cached greedy
    decode steps teacher-forced on the oracle's ids: every id identical, every oracle margin
    above twice the measured logit error."""
    d = R.CONFIGS["qwen3-0.6b"]
    s = span("qwen3-0.6b", 0, d.layers, True, True, "peaked")
    oracle = R.RefSpan(d, SEED, 0, d.layers - 1, True, True, torch.bfloat16, "sdpa", profile="peaked")
    prompt = torch.randint(0, d.vocab, (32,), generator=torch.Generator().manual_seed(5))
    ids = prompt.tolist()
    gpu_tokens, ref_tokens, margins = [], [], []
    lg_ref = oracle.forward_cached("s", prompt[None])[0, -1]
    out = s.forward([("s", 32)], ids=prompt, want_next_ids=True, want_logits=True, want_hidden=False)
    for step in range(12):
        gid = int(out["next_ids"][0])
        rid = int(torch.argmax(lg_ref))
        m = R.top2_margin(lg_ref)
        e = rel_err(out["logits"][0], lg_ref)
        ea = max_abs(out["logits"][0], lg_ref)
        gpu_tokens.append(gid)
        ref_tokens.append(rid)
        margins.append(m)
        print(f"step {step}: gpu {gid} ref {rid} margin {m:.4f} logits rel err {e:.2e}")
        assert e < 5e-2
        assert gid == rid, step
        assert m > 2 * ea, (step, m, ea)
        nxt = torch.tensor([rid])
        lg_ref = oracle.forward_cached("s", nxt[None])[0, -1]
        out = s.forward([("s", 1)], ids=nxt, want_next_ids=True, want_logits=True, want_hidden=False)
    print(f"greedy agreement {len(gpu_tokens)}/{len(gpu_tokens)}, smallest margin {min(margins):.2f}")


def test_weights_any_order():
    """The span's RMSNorms read their weights as set (reference rounding points, nothing folded
    at pack time): re-setting input_layernorm after the projections changes the output, and
    re-setting every weight restores the synthetic span bit for bit."""
    s = span("tiny", 0, 1, True, False)
    ids = torch.arange(8, dtype=torch.int32)
    ref = s.forward([(None, 8)], ids=ids)["hidden"].cpu()
    d = s.dims
    s.set_weight(0, "input_layernorm", torch.ones(d.hidden, dtype=torch.bfloat16) * 1.05)
    assert not torch.equal(s.forward([(None, 8)], ids=ids)["hidden"].cpu(), ref)
    s.init_synthetic(SEED)
    assert torch.equal(s.forward([(None, 8)], ids=ids)["hidden"].cpu(), ref)


def test_decode_fused_rope_vs_oracle():
    """Decode attention with QK-norm + RoPE + the cache write fused in (the only decode path):
    Qwen3-8B-dims heads (32 q / 8 kv), ragged contexts that put the new token at a page start,
    mid-page and page end; 5 decode steps each, every step against the oracle's cached forward
    (the cached K/V written in step k feed step k+1)."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["qwen3-8b"]
    lens = [63, 64, 100, 130]
    s = SpanRuntime(d, 0, 2, has_embed=True, has_lm_head=False, device=DEV, max_positions=1024,
                    kv_pages=32, max_tokens=512, max_seqs=4)
    s.init_synthetic(SEED)
    oracle = R.RefSpan(R.CONFIGS["qwen3-8b"], SEED, 0, 1, True, False, torch.bfloat16, "sdpa")
    prompts = [torch.randint(0, d.vocab, (n,), generator=torch.Generator().manual_seed(n)) for n in lens]
    s.forward([(f"s{i}", n) for i, n in enumerate(lens)], ids=torch.cat(prompts), want_hidden=False)
    for i, p in enumerate(prompts):
        oracle.forward_cached(f"s{i}", p[None])
    for step in range(5):
        ids = torch.tensor([(7 * step + 3 * i) % d.vocab for i in range(len(lens))])
        h = s.forward([(f"s{i}", 1) for i in range(len(lens))], ids=ids, want_hidden=True)["hidden"].cpu()
        ref = torch.cat([oracle.forward_cached(f"s{i}", ids[i].reshape(1, 1))[0] for i in range(len(lens))])
        e = rel_err(h, ref)
        print(f"fused decode step {step}: rel err {e:.2e}")
        assert e < TOL_REL


def test_decode_fused_long_context_vs_oracle():
    """The fused decode attention's long-context shape: from 96 cached pages per sequence the
    launcher takes 4-wave workgroups with more chunks (attention.hip decode_shape; here 24 per
    sequence and kv head), a path the 8B-dims test above does not reach.  Tiny-model span (n_rep 2,
    the q-staging prologue), two sequences whose new tokens land at a page start (6144) and
    mid-page (6200), 3 decode steps, every step's hidden states against the oracle's cached
    forward."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["tiny"]
    lens = [6144, 6200]
    s = SpanRuntime(d, 0, d.layers, has_embed=True, has_lm_head=False, device=DEV, max_positions=8192,
                    kv_pages=2 * 100 + 8, max_tokens=sum(lens), max_seqs=2)
    s.init_synthetic(SEED)
    oracle = R.RefSpan(R.CONFIGS["tiny"], SEED, 0, d.layers - 1, True, False, torch.bfloat16, "sdpa")
    prompts = [torch.randint(0, d.vocab, (n,), generator=torch.Generator().manual_seed(n)) for n in lens]
    s.forward([(f"s{i}", n) for i, n in enumerate(lens)], ids=torch.cat(prompts), want_hidden=False)
    for i, p in enumerate(prompts):
        oracle.forward_cached(f"s{i}", p[None])
    for step in range(3):
        ids = torch.tensor([(11 * step + 5 * i) % d.vocab for i in range(len(lens))])
        h = s.forward([(f"s{i}", 1) for i in range(len(lens))], ids=ids, want_hidden=True)["hidden"].cpu()
        ref = torch.cat([oracle.forward_cached(f"s{i}", ids[i].reshape(1, 1))[0] for i in range(len(lens))])
        e = rel_err(h, ref)
        print(f"fused long-context decode step {step}: rel err {e:.2e}")
        assert e < TOL_REL


@pytest.mark.parametrize("B", [4, 16, 40, 64])
def test_decode_packed_act_bit_exact(B):
    """The decode path's fragment-packed activations (residual stream, SwiGLU output, attention
    output) against the row-major layout the same span uses when per-layer outputs are
    requested (want_layers): same arithmetic in the same order, so the decode hidden states are
    bit-identical, for one (B <= 16) to four (B = 64) 16-row tiles and a partial last tile
    (B = 40)."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["qwen3-0.6b"]
    outs = []
    for layers in (False, True):
        s = SpanRuntime(d, 0, 2, has_embed=True, has_lm_head=False, device=DEV, max_positions=256,
                        kv_pages=2 * B + 4, max_tokens=64 * 8, max_seqs=B)
        s.init_synthetic(SEED)
        g = torch.Generator().manual_seed(B)
        ids = torch.randint(0, d.vocab, (B * 8,), generator=g)
        s.forward([(f"s{i}", 8) for i in range(B)], ids=ids, want_hidden=False)
        hs = []
        for step in range(3):
            nxt = torch.tensor([(5 * step + 11 * i) % d.vocab for i in range(B)])
            o = s.forward([(f"s{i}", 1) for i in range(B)], ids=nxt, want_hidden=True, want_layers=layers)
            hs.append(o["hidden"].cpu())
            if layers:
                assert torch.equal(o["layers"][-1].cpu(), hs[-1])
        outs.append(torch.stack(hs))
        del s
    assert torch.equal(outs[0], outs[1])


def test_config5_q32b_layer_prefill_vs_oracle():
    """BASELINE config 5 dims on the prefill path: one Qwen3-32B-dims layer (64 q / 8 kv
    heads, h 5120, I 25600) prefilling a 520-token prompt -- the ring-staged 256x256 GEMMs
    (M >= 512), the tail split (2 x 21 tiles), the 4-wave prefill attention and the
    QK-norm + RoPE kernel -- against the oracle layer, then 2 cached decode steps."""
    d = R.CONFIGS["qwen3-32b"]
    s = span("qwen3-32b", 9, 1, False, False, max_tokens=640, kv_pages=24, max_seqs=2, max_positions=1024)
    oracle = R.RefSpan(d, SEED, 9, 9, False, False, torch.bfloat16, "sdpa")
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(1, 520, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
    out = s.forward([("p", 520)], x=x[0])["hidden"]
    e = rel_err(out, oracle.forward_cached("p", x)[0])
    print(f"32B layer prefill 520: rel err {e:.2e}")
    assert e < TOL_REL
    for step in range(2):
        xd = (torch.randn(1, 1, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
        out = s.forward([("p", 1)], x=xd[0])["hidden"]
        e = rel_err(out, oracle.forward_cached("p", xd)[0])
        print(f"32B layer decode {step}: rel err {e:.2e}")
        assert e < TOL_REL


def test_prefill_qkv_epilogue_and_separate_kernel_vs_oracle():
    """q/k RMSNorm + RoPE and the K/V cache write in both of their homes, against the oracle:
    the persistent q/k/v GEMM's epilogue (a 780-row ragged prefill, >= 512 rows) and the
    separate qk_norm_rope_kv kernel (a 150-row cached extension, too short for the persistent
    GEMM), then a decode step reading the cache both wrote.  One Qwen3-8B-dims layer."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["qwen3-8b"]
    g = torch.Generator().manual_seed(9)
    x0 = (torch.randn(600 + 180, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
    x1 = (torch.randn(150, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
    x2 = (torch.randn(2, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
    oracle = R.RefSpan(R.CONFIGS["qwen3-8b"], SEED, 5, 5, False, False, torch.bfloat16, "sdpa")
    refs = [torch.cat([oracle.forward_cached("a", x0[None, :600])[0], oracle.forward_cached("b", x0[None, 600:])[0]]),
            oracle.forward_cached("a", x1[None])[0],
            torch.cat([oracle.forward_cached("a", x2[None, :1])[0], oracle.forward_cached("b", x2[None, 1:])[0]])]
    s = SpanRuntime(d, 5, 1, has_embed=False, has_lm_head=False, device=DEV, max_positions=1024,
                    kv_pages=40, max_tokens=1024, max_seqs=4)
    s.init_synthetic(SEED)
    outs = [s.forward([("a", 600), ("b", 180)], x=x0, want_hidden=True)["hidden"].cpu(),
            s.forward([("a", 150)], x=x1, want_hidden=True)["hidden"].cpu(),
            s.forward([("a", 1), ("b", 1)], x=x2, want_hidden=True)["hidden"].cpu()]
    for name, o, r in zip(("prefill 780 (GEMM epilogue)", "extension 150 (separate kernel)", "decode"), outs, refs):
        e = rel_err(o, r)
        print(f"{name}: vs oracle rel err {e:.2e}")
        assert e < TOL_REL


def test_prefill_qkv_epilogue_unaligned_slots_vs_oracle():
    """The q/k/v GEMM epilogue's V^T store takes 4 consecutive tokens per 8-byte store when their
    cache slots are consecutive and 4-aligned, else token by token: a sequence with 3 cached
    tokens extended by 600 (every group unaligned) beside a fresh 520-token one (aligned), then
    a decode step reading both caches.  One Qwen3-8B-dims layer against the oracle."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["qwen3-8b"]
    g = torch.Generator().manual_seed(11)
    x0 = (torch.randn(3, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
    x1 = (torch.randn(600 + 520, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
    x2 = (torch.randn(2, d.hidden, generator=g) * 0.5).to(torch.bfloat16)
    oracle = R.RefSpan(R.CONFIGS["qwen3-8b"], SEED, 5, 5, False, False, torch.bfloat16, "sdpa")
    oracle.forward_cached("c", x0[None])
    refs = [torch.cat([oracle.forward_cached("c", x1[None, :600])[0], oracle.forward_cached("d", x1[None, 600:])[0]]),
            torch.cat([oracle.forward_cached("c", x2[None, :1])[0], oracle.forward_cached("d", x2[None, 1:])[0]])]
    s = SpanRuntime(d, 5, 1, has_embed=False, has_lm_head=False, device=DEV, max_positions=1280,
                    kv_pages=48, max_tokens=1280, max_seqs=4)
    s.init_synthetic(SEED)
    s.forward([("c", 3)], x=x0, want_hidden=True)
    outs = [s.forward([("c", 600), ("d", 520)], x=x1, want_hidden=True)["hidden"].cpu(),
            s.forward([("c", 1), ("d", 1)], x=x2, want_hidden=True)["hidden"].cpu()]
    for name, o, r in zip(("prefill 1120 (unaligned + aligned V^T stores)", "decode"), outs, refs):
        e = rel_err(o, r)
        print(f"{name}: vs oracle rel err {e:.2e}")
        assert e < TOL_REL


def test_config3_q8b_layer_b16_ctx2048_decode_graph():
    """BASELINE config 3 at its full size, on the exact bench path: one Qwen3-8B layer,
    16 sequences prefilled with 2048 tokens each (two sequences per call, as bench.py does),
    then 3 decode steps as replays of the captured decode graph (split-K q/k/v GEMV, fused
    norm/RoPE/cache-write attention over 2k of paged context, o/gate-up/down GEMVs), each
    compared per sequence with the oracle's cached forward (bf16, SDPA) on the same inputs."""
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["qwen3-8b"]
    B, T, steps, layer = 16, 2048, 3, 5
    s = span("qwen3-8b", layer, 1, False, False, kv_pages=B * (T // 64 + 2) + 4, max_tokens=2 * T,
             max_seqs=B, max_positions=T + 64)
    oracle = R.RefSpan(d, SEED, layer, layer, False, False, torch.bfloat16, "sdpa")
    gen = torch.Generator().manual_seed(77)
    x = (torch.randn(B, T, d.hidden, generator=gen) * 0.5).to(torch.bfloat16)
    sess = [f"c3_{b}" for b in range(B)]
    worst = 0.0
    for b0 in range(0, B, 2):
        out = s.forward([(sid, T) for sid in sess[b0:b0 + 2]], x=x[b0:b0 + 2].reshape(2 * T, -1).to(DEV))["hidden"]
        for j in range(2):
            ref = oracle.forward_cached(sess[b0 + j], x[b0 + j:b0 + j + 1])[0]
            e = rel_err(out[j * T:(j + 1) * T], ref)
            worst = max(worst, e)
            assert e < TOL_REL, (b0 + j, e)
    print(f"prefill B={B} T={T}: worst rel err {worst:.2e}")
    xin = torch.zeros(B, d.hidden, dtype=torch.bfloat16, device=DEV)
    hout = torch.zeros(B, d.hidden, dtype=torch.bfloat16, device=DEV)
    g = DecodeGraph(s, sess, steps, x=xin, hidden_out=hout)
    for k in range(steps):
        xs = (torch.randn(B, d.hidden, generator=gen) * 0.5).to(torch.bfloat16)
        xin.copy_(xs.to(DEV))
        g.launch()
        torch.cuda.synchronize()
        got = hout.cpu()
        worst = 0.0
        for b in range(B):
            ref = oracle.forward_cached(sess[b], xs[b].reshape(1, 1, -1))[0, 0]
            e = rel_err(got[b], ref)
            worst = max(worst, e)
            assert e < TOL_REL, (k, b, e)
        print(f"decode step {k} (ctx {T + k + 1}): worst rel err {worst:.2e}")


def test_q8b_decode_ragged_contexts_vs_oracle():
    """Ragged decode batch at Qwen3-8B dims (one layer): 16 sequences whose cached lengths sit
    on and around page boundaries (1 .. 1500 tokens: 63/64/65, 127/128/129, 255/256/257 ...),
    so the decode attention sees 1..24 pages per sequence, chunk counts below the requested
    one, half-page items cut by the length mask and the writer's token on either side of a
    page edge; 3 eager decode steps then 3 decode-graph replays (each step crosses the edges
    of the 63/127/255-token sequences), every sequence's hidden state against the oracle's
    cached forward (Qwen3Server.send semantics)."""
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["qwen3-8b"]
    lens = [1, 2, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 700, 1000, 1500]
    B, layer = len(lens), 3
    s = span("qwen3-8b", layer, 1, False, False, kv_pages=sum(n // 64 + 2 for n in lens) + 8, max_tokens=1600,
             max_seqs=B, max_positions=1600)
    oracle = R.RefSpan(d, SEED, layer, layer, False, False, torch.bfloat16, "sdpa")
    gen = torch.Generator().manual_seed(31)
    sess = [f"r{i}" for i in range(B)]
    for sid, n in zip(sess, lens):
        x0 = (torch.randn(1, n, d.hidden, generator=gen) * 0.5).to(torch.bfloat16)
        s.forward([(sid, n)], x=x0[0].to(DEV))
        oracle.forward_cached(sid, x0)
    worst = 0.0
    xin = torch.zeros(B, d.hidden, dtype=torch.bfloat16, device=DEV)
    hout = torch.zeros(B, d.hidden, dtype=torch.bfloat16, device=DEV)
    for step in range(6):
        xs = (torch.randn(B, d.hidden, generator=gen) * 0.5).to(torch.bfloat16)
        if step < 3:
            got = s.forward([(sid, 1) for sid in sess], x=xs.to(DEV))["hidden"].cpu()
        else:
            if step == 3:
                g = DecodeGraph(s, sess, 3, x=xin, hidden_out=hout)
            xin.copy_(xs.to(DEV))
            g.launch()
            torch.cuda.synchronize()
            got = hout.cpu()
        for b in range(B):
            ref = oracle.forward_cached(sess[b], xs[b].reshape(1, 1, -1))[0, 0]
            e = rel_err(got[b], ref)
            worst = max(worst, e)
            assert e < TOL_REL, (step, lens[b], e)
    s.check_errors()
    print(f"ragged decode, 16 sequences of 1..1500 cached tokens, 6 steps: worst rel err {worst:.2e}")


def test_eager_step_equals_graph_replay():
    """DecodeGraph.launch_eager (inferd_span_step: the replay's scheduler step and forward
    launched kernel by kernel) walks the sequences exactly as graph replays do: two identical
    Qwen3-0.6B 2-layer spans, one replaying its graph and one stepping eagerly, give bit-identical
    hidden states over 6 steps, with the steps interleaved on the eager span too."""
    from inferd_amd.runtime import DecodeGraph
    d = R.CONFIGS["qwen3-0.6b"]
    B, T, STEPS = 3, 20, 6
    gen = torch.Generator().manual_seed(51)
    x_pre = (torch.randn(B * T, d.hidden, generator=gen) * 0.5).to(torch.bfloat16)
    steps = [(torch.randn(B, d.hidden, generator=gen) * 0.5).to(torch.bfloat16) for _ in range(STEPS)]
    outs = []
    for mode in ("graph", "eager", "mixed"):
        s = span("qwen3-0.6b", 3, 2, False, False, kv_pages=8, max_tokens=B * T, max_seqs=B, max_positions=256)
        sess = [f"e{b}" for b in range(B)]
        s.forward([(sid, T) for sid in sess], x=x_pre.to(DEV), want_hidden=False)
        xin = torch.zeros(B, d.hidden, dtype=torch.bfloat16, device=DEV)
        hout = torch.zeros(B, d.hidden, dtype=torch.bfloat16, device=DEV)
        g = DecodeGraph(s, sess, STEPS, x=xin, hidden_out=hout)
        seq = []
        for k in range(STEPS):
            xin.copy_(steps[k])
            eager = mode == "eager" or (mode == "mixed" and k % 2)
            (g.launch_eager if eager else g.launch)()
            seq.append(hout.cpu().clone())
        s.check_errors()
        outs.append(torch.stack(seq))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_record_boundaries_refuse_multi_call_forwards():
    """A forward whose hand-off is a record is one engine call: an attention|o span refuses a
    request larger than its workspace (chunked prefill would need one record per chunk), and a span
    ending before o always hands over its record (want_hidden=False refused)."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["qwen3-0.6b"]
    so = SpanRuntime(d, 1, 2, has_embed=False, has_lm_head=False, device=DEV, kv_pages=16, max_tokens=64,
                     max_seqs=4, o_split_last=True)
    so.init_synthetic(SEED)
    x = torch.zeros(100, d.hidden, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="one engine call"):
        so.forward([("a", 100)], x=x)
    with pytest.raises(ValueError, match="always hands over its record"):
        so.forward([("b", 10)], x=x[:10], want_hidden=False)
    out = so.forward([("c", 10)], x=x[:10])
    assert out["record"].numel() == 10 * d.hidden + 10 * d.heads * d.head_dim


def test_c_host_span_greedy():
    """The drop-in boundary without Python: tests/c_abi/span_host.c (plain C over
    include/inferd_span.h and HIP's C API; no Python or torch in its process, built by
    __graft_entry__.build()) prefills B sessions in one call through the native page table and
    decodes greedily, one forward call per step for all B.  Every id equals the torch extension's
    run of the same span (SpanRuntime: same seed, prompts and batching; the kernels are
    deterministic), on the tiny model and on Qwen3-0.6B (config 2's model)."""
    from inferd_amd.runtime import MODELS, SpanRuntime
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "c_abi", "span_host")
    assert os.path.exists(exe), "tests/c_abi/span_host is not built (__graft_entry__.build())"
    for model, B, T, steps in (("tiny", 3, 21, 6), ("qwen3-0.6b", 2, 70, 5)):
        r = subprocess.run([exe, model, str(SEED), str(B), str(T), str(steps)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)
        c_ids = [[int(v) for v in line.split(":")[1].split()] for line in r.stdout.splitlines()
                 if line.startswith("ids ")]
        d = MODELS[model]
        s = SpanRuntime(d, 0, d.layers, has_embed=True, has_lm_head=True, device=DEV, max_positions=8192,
                        kv_pages=B * ((T + steps + 63) // 64) + 8, max_tokens=B * T, max_seqs=B)
        s.init_synthetic(SEED)
        prompt = torch.tensor([(7919 * t + 104729 * b + 17) % d.vocab for b in range(B) for t in range(T)])
        out = s.forward([(f"c{b}", T) for b in range(B)], ids=prompt, want_next_ids=True, want_hidden=False)
        ids = [out["next_ids"].cpu().tolist()]
        for _ in range(steps):
            out = s.forward([(f"c{b}", 1) for b in range(B)], ids=torch.tensor(ids[-1]), want_next_ids=True,
                            want_hidden=False)
            ids.append(out["next_ids"].cpu().tolist())
        torch_ids = [[ids[k][b] for k in range(steps + 1)] for b in range(B)]
        print(f"{model}: C host {c_ids}, torch {torch_ids}")
        assert c_ids == torch_ids, model
        s.release_all()


@pytest.mark.parametrize("name,hidden,inter,heads,kv", [("qwen3-1.7b", 2048, 6144, 16, 8),
                                                       ("qwen3-4b", 2560, 9728, 32, 8),
                                                       ("qwen3-14b", 5120, 17408, 40, 8)])
def test_other_qwen3_sizes_layer_vs_oracle(name, hidden, inter, heads, kv):
    """Qwen3 sizes the bench does not run, which split_model.checkpoint_dims now loads from a
    checkpoint's config.json (public Qwen3 configs): one layer of each, a ragged 600 + 77-token
    prefill (the persistent prefill GEMMs on partial tiles) then 3 cached decode steps (the decode
    GEMVs at these K / N; at 14B, 5 query heads per kv head: the fused decode attention without
    the q-staging prologue), every output against the oracle at the span tolerance."""
    from inferd_amd.runtime import ModelDims, SpanRuntime
    d = ModelDims(name, hidden, inter, heads, kv, 1, 151936)
    od = R.Qwen3Dims(name, hidden, inter, heads, kv, 1, 151936)
    s = SpanRuntime(d, 0, 1, has_embed=False, has_lm_head=False, device=DEV, max_positions=1024, kv_pages=24,
                    max_tokens=700, max_seqs=2)
    s.init_synthetic(SEED)
    oracle = R.RefSpan(od, SEED, 0, 0, False, False, torch.bfloat16, "sdpa")
    g = torch.Generator().manual_seed(3)
    lens = [600, 77]
    xs = [(torch.randn(n, hidden, generator=g) * 0.5).to(torch.bfloat16) for n in lens]
    h = s.forward([(f"s{i}", n) for i, n in enumerate(lens)], x=torch.cat(xs))["hidden"].cpu()
    ref = torch.cat([oracle.forward_cached(f"s{i}", x[None])[0] for i, x in enumerate(xs)])
    e = rel_err(h, ref)
    print(f"{name} prefill: rel err {e:.2e}")
    assert e < TOL_REL
    for step in range(3):
        xd = [(torch.randn(1, hidden, generator=g) * 0.5).to(torch.bfloat16) for _ in lens]
        h = s.forward([(f"s{i}", 1) for i in range(len(lens))], x=torch.cat(xd))["hidden"].cpu()
        ref = torch.cat([oracle.forward_cached(f"s{i}", x[None])[0] for i, x in enumerate(xd)])
        e = rel_err(h, ref)
        print(f"{name} decode step {step}: rel err {e:.2e}")
        assert e < TOL_REL
    s.release_all()
