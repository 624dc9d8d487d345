"""GPU tests of sampled decoding (inferd_amd/csrc/sampling.hip behind inferd_sample, the span's
sampled head, DecodeGraph and PartitionedQwen2's "sampling" key) against the fp64 numpy reference
of the draw (tests/sampling_ref.py).  Ids must equal the reference on every decidable case; a test
may leave out at most 5 % of its cases as undecidable (sampling_ref: u or a top-p tail sum within
2e-5 of a boundary).  The span tests apply the reference to each call's own returned logits, so
they do not depend on the model's numerics."""
import numpy as np
import pytest
import torch

import sampling_ref as SR

pytestmark = pytest.mark.gpu

SEED = 1234
DRAW_SEED = 20240607
POSITIONS = (0, 1, 2, 63, 64, 2047, 8191, 40959)
DEV = "cuda:0"
_DISTS = {}


def _dists(tag, logits_np, T, k, p):
    """the rows' reference distributions, computed once per (input, parameter set)"""
    key = (tag, T, k, p)
    if key not in _DISTS:
        _DISTS[key] = [SR.RowDist(logits_np[r], T, k, p) for r in range(logits_np.shape[0])]
    return _DISTS[key]


def _ref_ids(dists, seed, row_seeds, positions):
    ids, dec = [], []
    for d, rs, pos in zip(dists, row_seeds, positions):
        i, ok = d.draw(SR.uniform(seed, int(rs), int(pos)))
        ids.append(i)
        dec.append(ok)
    return np.array(ids, dtype=np.int32), np.array(dec)


def _row_seeds(n):
    return [(0x9E3779B97F4A7C15 * (r + 1) + 0xDEADBEEF) % 2 ** 64 for r in range(n)]


def test_single_op_uniform_bits():
    """u_out is the numpy counter generator's uniform bit for bit: 64 rows, positions including 0
    and 40,959, with the row index and with explicit 64-bit row seeds."""
    from inferd_amd.runtime import sample
    lg = SR.bf16_logits(64, 1024).to(DEV)
    pos = [POSITIONS[r % 8] for r in range(64)]
    for rs in (None, _row_seeds(64)):
        ids, u = sample(lg, 0.6, 20, 0.95, DRAW_SEED, pos, row_seeds=rs, want_u=True)
        want = SR.uniforms(DRAW_SEED, range(64) if rs is None else rs, pos)
        assert np.array_equal(u.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert 0 <= int(ids.min()) and int(ids.max()) < 1024


@pytest.mark.parametrize("vocab", [48, 1024, 151936])
def test_single_op_ids_match_reference(vocab):
    """rows 1 / 16 / 64, the four parameter sets, with and without row_seeds, two position
    assignments: exact ids on every decidable case, at most 5 % undecidable, no overflow flag."""
    from inferd_amd.runtime import sample
    lg_cpu = SR.bf16_logits(64, vocab)
    lg_np = lg_cpu.float().numpy()
    lg = lg_cpu.to(DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    cases = undecided = 0
    for T, k, p in SR.PARAM_SETS:
        dists = _dists(("randn", vocab), lg_np, T, k, p)
        for rows in (1, 16, 64):
            for shift, rs in ((0, None), (3, _row_seeds(rows))):
                pos = [POSITIONS[(r + shift) % 8] for r in range(rows)]
                got = sample(lg[:rows], T, k, p, DRAW_SEED, pos, row_seeds=rs, flags=flags).cpu().numpy()
                want, dec = _ref_ids(dists[:rows], DRAW_SEED, range(rows) if rs is None else rs, pos)
                bad = np.nonzero(dec & (got != want))[0]
                assert bad.size == 0, (T, k, p, rows, rs is not None, bad[:8], got[bad[:8]], want[bad[:8]])
                cases += rows
                undecided += int((~dec).sum())
    print(f"vocab {vocab}: {cases} cases, {undecided} undecidable")
    assert undecided <= 0.05 * cases
    assert int(flags.item()) == 0


def test_non_finite_rows_yield_in_range_ids():
    """NaN logits have no defined draw; the kernel still writes a column inside the vocabulary
    (all-NaN rows, a NaN inside the top tile, k = 1 and k = 20), and finite rows beside them are
    drawn as the reference draws them."""
    from inferd_amd.runtime import sample
    lg = SR.bf16_logits(4, 1024).float()
    ref_row = lg[3].numpy().copy()
    lg[0, :] = float("nan")
    lg[1, int(lg[1].argmax())] = float("nan")
    lg[2, 5] = float("nan")
    for T, k, p in ((0.6, 20, 0.95), (1.0, 1, 1.0), (1.0, 64, 1.0)):
        ids = sample(lg.to(torch.bfloat16).to(DEV), T, k, p, DRAW_SEED, [7, 8, 9, 10]).cpu().numpy()
        assert ((ids >= 0) & (ids < 1024)).all(), ids
        want, dec, _ = SR.sample_row(ref_row, T, k, p, SR.uniform(DRAW_SEED, 3, 10))
        assert not dec or ids[3] == want


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def test_single_op_crafted_rows():
    """One dominant logit (kept set of 1), an exact tie straddling the k-th value, the maximum in
    the last / first tile; at V = 4096 all-equal logits and three distinct values over equal ones
    (the capacity rule: the reference's ids, flag bit 2), and the whole top-k inside one tile over
    equal logits (more candidate columns than the kernel's list, no overflow)."""
    from inferd_amd.runtime import sample
    a = np.concatenate([SR.crafted_rows(1024, k=20)[[0, 1, 3, 4]], SR.crafted_rows(1024, k=64)[[1]]])
    cases = undecided = 0
    for tag, rows_np, overflow in (("crafted1024", a, False), ("cap4096", _capacity_rows(), True),
                                   ("onetile4096", _one_tile_rows(), False)):
        lg = _bf16(rows_np).to(DEV)
        assert np.array_equal(lg.float().cpu().numpy(), rows_np)          # bf16-exact inputs
        n = rows_np.shape[0]
        for T, k, p in SR.PARAM_SETS + ((0.6, 4, 1.0),):
            dists = _dists(tag, rows_np, T, k, p)
            for pos0 in (0, 5, 77, 4000):
                pos = [pos0 + r for r in range(n)]
                flags = torch.zeros(1, dtype=torch.int32, device=DEV)
                got = sample(lg, T, k, p, DRAW_SEED, pos, flags=flags).cpu().numpy()
                want, dec = _ref_ids(dists, DRAW_SEED, range(n), pos)
                bad = np.nonzero(dec & (got != want))[0]
                assert bad.size == 0, (tag, T, k, p, pos0, bad, got[bad], want[bad])
                ovf = any(d.overflow for d in dists)
                assert int(flags.item()) == (4 if ovf else 0), (tag, T, k, p)
                if tag != "onetile4096":
                    assert ovf == overflow
                cases += n
                undecided += int((~dec).sum())
    d = _dists("crafted1024", a, 0.6, 20, 0.95)
    assert d[0].kept.size == 1 and d[1].n_topk == 24 and _dists("crafted1024", a, 1.5, 64, 0.5)[4].n_topk > 64
    assert undecided <= 0.05 * cases, (undecided, cases)


def _capacity_rows():
    r = np.full((2, 4096), 1.5, dtype=np.float32)
    r[1, [5, 2000, 4095]] = [4.0, 3.0, 2.0]
    return r


def _one_tile_rows():
    """rows whose 16 largest values share one 16-column tile, every other column equal"""
    r = np.full((2, 4096), -1.0, dtype=np.float32)
    r[0, 32:48] = np.arange(16, dtype=np.float32) * 0.25 + 1.0
    r[1, 4080:4096] = np.arange(16, 0, -1, dtype=np.float32) * 0.5
    return r


# ------------------------------------------------------------------ span
def _tiny_span(profile="random"):
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["tiny"]
    s = SpanRuntime(d, 0, d.layers, has_embed=True, has_lm_head=True, device=DEV, kv_pages=16, max_tokens=256,
                    max_seqs=4, max_positions=1024)
    s.init_synthetic(SEED, profile)
    return s


def _check_call(out, params, row_seeds, positions, stats):
    lg = out["logits"].float().cpu().numpy()
    got = out["next_ids"].cpu().numpy()
    for r in range(lg.shape[0]):
        want, dec, _ = SR.sample_row(lg[r], *params, SR.uniform(DRAW_SEED, row_seeds[r], positions[r]))
        stats[0] += 1
        stats[1] += not dec
        assert not dec or got[r] == want, (r, positions[r], got[r], want)


LENS = (1, 17, 65)


def test_span_prefill_and_decode_match_reference_on_own_logits():
    """tiny geometry (vocab 1024), one span with embed and lm_head: a ragged prefill of 3 sessions
    (1, 17 and 65 tokens) then 8 decode steps, every call's sampled ids = the reference applied to
    that call's returned logits; after clear_sampling the ids are argmax of the logits again."""
    s = _tiny_span()
    params = (0.6, 20, 0.95)
    rs = _row_seeds(3)
    s.set_sampling(*params, DRAW_SEED, row_seeds=rs)
    prompt = torch.randint(0, 1024, (sum(LENS),), generator=torch.Generator().manual_seed(3))
    stats = [0, 0]
    out = s.forward([(f"s{i}", n) for i, n in enumerate(LENS)], ids=prompt, want_hidden=False, want_next_ids=True,
                    want_logits=True)
    _check_call(out, params, rs, list(LENS), stats)
    # the same call without a logits output (the span's own logits buffer) draws the same ids
    s2 = _tiny_span()
    s2.set_sampling(*params, DRAW_SEED, row_seeds=rs)
    out2 = s2.forward([(f"s{i}", n) for i, n in enumerate(LENS)], ids=prompt, want_hidden=False, want_next_ids=True)
    assert torch.equal(out2["next_ids"], out["next_ids"])
    for step in range(8):
        out = s.forward([(f"s{i}", 1) for i in range(3)], ids=out["next_ids"], want_hidden=False, want_next_ids=True,
                        want_logits=True)
        _check_call(out, params, rs, [n + step + 1 for n in LENS], stats)
    assert stats[1] <= 0.05 * stats[0], stats
    s.check_errors()
    s.clear_sampling()
    out = s.forward([(f"s{i}", 1) for i in range(3)], ids=out["next_ids"], want_hidden=False, want_next_ids=True,
                    want_logits=True)
    assert torch.equal(out["next_ids"].long(), torch.argmax(out["logits"].float(), dim=-1))


@pytest.mark.parametrize("seeded", [True, False])
def test_forward_cut_into_engine_calls_keeps_each_requests_row_seed(seeded):
    """A forward whose requests exceed the span's workspace runs as several engine calls (here
    max_tokens 32 / max_seqs 2: requests of 20, 20, 20 and 5 tokens end in three engine calls,
    requests 1 and 2 as rows 0 and 1 of the second, request 3 as row 0 of the third): every request
    still draws with ITS row seed (its index without row_seeds), checked against the reference on
    the returned logits; the same requests in one engine call likewise.  Afterwards the setting is
    back on the whole list.  Fewer seeds than sequences: ValueError from forward and DecodeGraph."""
    from inferd_amd.runtime import MODELS, DecodeGraph, SpanRuntime
    d = MODELS["tiny"]
    lens = (20, 20, 20, 5)
    params = (1.0, 64, 1.0)
    rs = _row_seeds(4) if seeded else None
    prompt = torch.randint(0, 1024, (sum(lens),), generator=torch.Generator().manual_seed(6))
    for max_tokens, max_seqs in ((32, 2), (256, 4)):
        s = SpanRuntime(d, 0, d.layers, has_embed=True, has_lm_head=True, device=DEV, kv_pages=16,
                        max_tokens=max_tokens, max_seqs=max_seqs, max_positions=1024)
        s.init_synthetic(SEED)
        s.set_sampling(*params, DRAW_SEED, row_seeds=rs)
        reqs = [(f"s{i}", n) for i, n in enumerate(lens)]
        assert len(s._plan(reqs)) == (3 if max_tokens == 32 else 1)
        out = s.forward(reqs, ids=prompt, want_hidden=False, want_next_ids=True, want_logits=True)
        stats = [0, 0]
        _check_call(out, params, rs if seeded else list(range(4)), list(lens), stats)
        assert stats[1] == 0, stats
        s.check_errors()
        if seeded:      # the setting itself is back on the whole list after the cut call
            nxt = s.forward([(f"s{i}", 1) for i in (0, 1)], ids=out["next_ids"][:2], want_hidden=False,
                            want_next_ids=True, want_logits=True)
            _check_call(nxt, params, rs, [n + 1 for n in lens[:2]], stats)
            assert stats[1] == 0, stats
            s.set_sampling(*params, DRAW_SEED, row_seeds=rs[:1])
            with pytest.raises(ValueError, match="row_seeds"):
                s.forward([("s0", 1), ("s1", 1)], ids=nxt["next_ids"], want_hidden=False, want_next_ids=True)
            with pytest.raises(ValueError, match="row_seeds"):
                cur = nxt["next_ids"].clone()
                DecodeGraph(s, ["s0", "s1"], 2, ids=cur, next_ids=cur)


def test_decode_graph_samples_like_eager_steps():
    """8 steps as DecodeGraph.launch() with ids aliasing next_ids = the same 8 steps as launch_eager()
    from the same state, and = the reference on each replay's logits (the draw is at the position
    the token will occupy, read on the device)."""
    from inferd_amd.runtime import DecodeGraph
    params = (1.5, 64, 0.5)
    rs = _row_seeds(3)
    prompt = torch.randint(0, 1024, (sum(LENS),), generator=torch.Generator().manual_seed(4))
    spans, curs, graphs = [], [], []
    lgbuf = torch.zeros(3, 1024, dtype=torch.bfloat16, device=DEV)
    for which in range(2):
        s = _tiny_span()
        s.set_sampling(*params, DRAW_SEED, row_seeds=rs)
        out = s.forward([(f"s{i}", n) for i, n in enumerate(LENS)], ids=prompt, want_hidden=False,
                        want_next_ids=True)
        cur = out["next_ids"].clone()
        graphs.append(DecodeGraph(s, [f"s{i}" for i in range(3)], 8, ids=cur, next_ids=cur,
                                  logits=lgbuf if which == 0 else None))
        spans.append(s)
        curs.append(cur)
    assert torch.equal(curs[0], curs[1])
    spans[0].clear_sampling()          # the setting is baked into the captured graph
    stats = [0, 0]
    for step in range(8):
        graphs[0].launch()
        graphs[1].launch_eager()
        torch.cuda.synchronize()
        assert torch.equal(curs[0], curs[1]), step
        _check_call({"logits": lgbuf, "next_ids": curs[0]}, params, rs, [n + step + 1 for n in LENS], stats)
    assert stats[1] <= 0.05 * stats[0], stats
    for s in spans:
        s.check_errors()


def test_top_k_1_is_greedy_on_the_peaked_profile():
    s = _tiny_span("peaked")
    prompt = torch.randint(0, 1024, (sum(LENS),), generator=torch.Generator().manual_seed(5))
    greedy = s.forward([(f"g{i}", n) for i, n in enumerate(LENS)], ids=prompt, want_hidden=False, want_next_ids=True)
    s.set_sampling(1.0, 1, 1.0, DRAW_SEED)
    drawn = s.forward([(f"s{i}", n) for i, n in enumerate(LENS)], ids=prompt, want_hidden=False, want_next_ids=True)
    assert torch.equal(greedy["next_ids"], drawn["next_ids"])
    for _ in range(4):
        s.clear_sampling()
        greedy = s.forward([(f"g{i}", 1) for i in range(3)], ids=greedy["next_ids"], want_hidden=False,
                           want_next_ids=True)
        s.set_sampling(1.0, 1, 1.0, DRAW_SEED)
        drawn = s.forward([(f"s{i}", 1) for i in range(3)], ids=drawn["next_ids"], want_hidden=False,
                          want_next_ids=True)
        assert torch.equal(greedy["next_ids"], drawn["next_ids"])


def test_set_sampling_refusals():
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["tiny"]
    first = SpanRuntime(d, 0, 2, has_embed=True, has_lm_head=False, device=DEV, kv_pages=16, max_tokens=64,
                        max_seqs=4, max_positions=1024)
    with pytest.raises(ValueError, match="lm_head"):
        first.set_sampling(0.6, 20, 0.95, 1)
    with pytest.raises(RuntimeError, match="lm_head"):
        torch.ops.inferd.span_set_sampling(first.handle, 0.6, 20, 0.95, 1, None, True)
    s = _tiny_span()
    for bad in ((0.0, 20, 0.95), (0.6, 65, 0.95), (0.6, 20, 0.0)):
        with pytest.raises(ValueError):
            s.set_sampling(*bad, 1)
    assert s.sampling is None


# ------------------------------------------------------------------ PartitionedQwen2
def test_partitioned_chain_samples(tmp_path):
    """Two PartitionedQwen2 stages on tiny converted parts: a session with "sampling" reproduces
    itself when replayed with the same seed, differs from the greedy chain where the reference says
    it must, and every token is the reference's draw on the last stage's logits; a stateless call
    draws with row seed 0."""
    from hf_fixtures import write_reference_parts
    from inferd_amd.convert_parts import convert
    from inferd_amd.partitioned_models import PartitionedQwen2, session_row_seed
    from inferd_amd.runtime import MODELS
    from oracle import qwen3_ref as R
    cfg = {"model_name": "tiny", "parts_dir": str(tmp_path / "parts"), "stages_count": 2,
           "stages": [{"name": "node0", "stage": 0, "start_layer": 0, "end_layer": 1},
                      {"name": "node1", "stage": 1, "start_layer": 2, "end_layer": 3}]}
    write_reference_parts(tmp_path / "parts", cfg, R.CONFIGS["tiny"], SEED)
    paths = convert(cfg, MODELS["tiny"], str(tmp_path / "parts"), str(tmp_path / "converted"))
    n0, n1 = PartitionedQwen2("tiny", 2, 0, paths[0]), PartitionedQwen2("tiny", 2, 1, paths[1])
    prompt = list(range(3, 60, 3))
    params = (1.0, 64, 1.0)

    def chain(sid, sampling, steps=6):
        ids, toks, lgs = list(prompt), [], []
        for _ in range(steps):
            req = {"generated_ids": ids, "session_id": sid}
            if sampling:
                req["sampling"] = sampling
            mid = n0.forward(req)
            assert ("sampling" in mid) == bool(sampling)
            res = n1.forward(mid)
            assert "sampling" not in res
            toks.append(res["next_token_id"])
            lgs.append(n1.model.last_logits[0].float().cpu().numpy())
            ids = res["generated_ids"]
        for n in (n0, n1):
            n.close_session(sid)
        return toks, lgs

    greedy, g_lgs = chain("greedy", None)
    assert greedy == [int(np.argmax(l)) for l in g_lgs]
    rseed = session_row_seed("chat")
    # a seed under which the reference's first draw (on the greedy chain's first logits: the same
    # prompt) is not the argmax
    def differs(sd):
        want, dec, _ = SR.sample_row(g_lgs[0], *params, SR.uniform(sd, rseed, len(prompt)))
        return dec and want != greedy[0]
    seed = next(sd for sd in range(100, 200) if differs(sd))
    sampling = dict(zip(("temperature", "top_k", "top_p"), params), seed=seed)
    toks, lgs = chain("chat", sampling)
    again, _ = chain("chat", sampling)
    assert toks == again
    assert toks != greedy and toks[0] != greedy[0]
    undecided = 0
    for i, (t, l) in enumerate(zip(toks, lgs)):
        want, dec, _ = SR.sample_row(l, *params, SR.uniform(seed, rseed, len(prompt) + i))
        undecided += not dec
        assert not dec or t == want, (i, t, want)
    # stateless: row seed 0, the position is the prompt's length; the answer after it is greedy again
    mid = n0.forward({"generated_ids": prompt, "sampling": sampling})
    res = n1.forward(mid)
    want, dec, _ = SR.sample_row(n1.model.last_logits[0].float().cpu().numpy(), *params,
                                 SR.uniform(seed, 0, len(prompt)))
    assert not dec or res["next_token_id"] == want
    undecided += not dec
    assert undecided <= 0.05 * (len(toks) + 1)
    assert n1.forward(n0.forward({"generated_ids": prompt}))["next_token_id"] == greedy[0]
    with pytest.raises(ValueError, match="top_k"):
        n0.forward({"generated_ids": prompt, "sampling": {**sampling, "top_k": 0}})
    with pytest.raises(ValueError, match="sampling"):
        n1.forward({**mid, "sampling": {"temperature": 1.0}})
