"""GPU tests of the sampled vocab-parallel head (sample_shard_kernel in inferd_amd/csrc/sampling.hip
behind inferd_sample_shard / inferd_span_head_shard_sampled, and PipelineStage(sampling=...)).

The claim is bit identity with the whole head: a chain of shard calls over any partition of the
vocabulary, in any order, ends in the ids, uniforms and overflow flag of inferd_sample on the whole
row (runtime.sample / a has_lm_head span under set_sampling).  The intermediate records are compared
with the numpy restatement (tests/sampling_shard_ref.py) word for word, and the ids with the fp64
reference of the draw (tests/sampling_ref.py) on every decidable case."""
import numpy as np
import pytest
import torch

import sampling_ref as SR
import sampling_shard_ref as SH

pytestmark = pytest.mark.gpu

SEED = 1234
DRAW_SEED = 20240607
POSITIONS = (0, 1, 2, 63, 64, 2047, 8191, 40959)
DEV = "cuda:0"


def _row_seeds(n):
    return [(0x9E3779B97F4A7C15 * (r + 1) + 0xDEADBEEF) % 2 ** 64 for r in range(n)]


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def _chain(lg, bounds, order, params, pos, rs, flags=None, records=None, finisher=False):
    """sample_shard chained over the shards of `order`; the last call draws -- or, with finisher, a
    call of its own over no columns does.  records: list receiving each call's cand_out (numpy)."""
    from inferd_amd.runtime import cand_record, sample_shard
    T, k, p = params
    rows = lg.shape[0]
    rec, out = None, None
    for j, i in enumerate(order):
        a, b = bounds[i], bounds[i + 1]
        last = j == len(order) - 1 and not finisher
        part = lg[:, a:b].contiguous()                  # an empty shard: [rows, 0]
        new = cand_record(rows, lg.device)
        new.fill_(-1)                                   # every word must be written
        out = sample_shard(part, a, T, k, p, DRAW_SEED, rows=rows, cand_in=rec, cand_out=new,
                           positions=pos if last else None, row_seeds=rs, want_ids=last, want_u=last, flags=flags)
        rec = new
        if records is not None:
            records.append(rec.cpu().numpy().view(np.uint64))
    if finisher:
        out = sample_shard(None, bounds[-1], T, k, p, DRAW_SEED, rows=rows, cand_in=rec, positions=pos, row_seeds=rs,
                           want_ids=True, want_u=True, flags=flags)
    return out


def _orders(n):
    sh = list(np.random.RandomState(n).permutation(n))
    return [list(range(n)), sh if sh != list(range(n)) else sh[::-1]]


@pytest.mark.parametrize("vocab", [1024, 151936])
def test_single_op_chain_equals_whole_head(vocab):
    """64 random rows, the four parameter sets, five partitions (a 16-column shard, uneven parts, an
    empty shard), stage order and a shuffled order: ids, u and the flag of the chain = runtime.sample
    on the whole logits bit for bit; every intermediate record = the numpy record; the ids = the fp64
    reference on every decidable case (at most 5 % undecidable)."""
    from inferd_amd.runtime import sample
    lg_cpu = SR.bf16_logits(64, vocab)
    lg_np = lg_cpu.float().numpy()
    lg = lg_cpu.to(DEV)
    pos = [POSITIONS[r % 8] for r in range(64)]
    rs = _row_seeds(64)
    cases = undecided = 0
    for T, k, p in SR.PARAM_SETS:
        wflags = torch.zeros(1, dtype=torch.int32, device=DEV)
        wid, wu = sample(lg, T, k, p, DRAW_SEED, pos, row_seeds=rs, want_u=True, flags=wflags)
        keys = SH.entry_keys(lg_np, T)
        ref_ids, dec, ovf = SR.sample_rows(lg_np, T, k, p, DRAW_SEED, pos, rs)
        bad = np.nonzero(dec & (wid.cpu().numpy() != ref_ids))[0]
        assert bad.size == 0, (T, k, p, bad[:8])
        cases += 64
        undecided += int((~dec).sum())
        for ci, parts in enumerate(SH.cuts(vocab)):
            b = SH.bounds_of(parts)
            for order in _orders(len(parts)):
                flags = torch.zeros(1, dtype=torch.int32, device=DEV)
                recs = [] if (ci + len(order)) % 2 == 0 or vocab == 1024 else None
                ids, u = _chain(lg, b, order, (T, k, p), pos, rs, flags, recs)
                assert torch.equal(ids, wid), (T, k, p, parts, order)
                assert torch.equal(u.view(torch.int32), wu.view(torch.int32))
                assert int(flags.item()) == int(wflags.item()) == (4 if ovf.any() else 0)
                if recs is not None:
                    for r in range(0, 64, 1 if vocab == 1024 else 8):
                        want = SH.chain(keys[r], b, order, k)
                        for j in range(len(order)):
                            assert np.array_equal(recs[j][r], want[j]), (T, k, p, parts, order, r, j)
    print(f"vocab {vocab}: {cases} cases, {undecided} undecidable")
    assert undecided <= 0.05 * cases


def _capacity_rows():
    r = np.full((2, 4096), 1.5, dtype=np.float32)
    r[1, [5, 2000, 4095]] = [4.0, 3.0, 2.0]
    return r


def _boundary_row(n_equal, vocab=4096):
    row = np.full(vocab, -8.0, dtype=np.float32)
    first = n_equal // 2
    row[np.arange(first) * 3 % 2048] = 1.5
    row[2048 + np.arange(n_equal - first) * 5 % 2048] = 1.5
    assert int((row == 1.5).sum()) == n_equal
    return row


def test_crafted_rows_mass_ties_and_capacity_boundary():
    """sampling_ref.crafted_rows(4096) (a dominant logit, ties across the k-th value, ALL-EQUAL logits:
    more candidates than the list holds in each shard -- the mass-ties path -- and capacity overflow,
    maxima in the first / last tile), two more all-equal-based rows, and rows with exactly 256 and 257
    qualifying columns, cut [2048, 2048] and [16, 4080] in both orders and with a finishing call over
    no columns: ids, u, the flag per row set and the records as the whole head / numpy have them."""
    from inferd_amd.runtime import sample
    sets = (("crafted", SR.crafted_rows(4096), True), ("cap", _capacity_rows(), True),
            ("b256", _boundary_row(256)[None], False), ("b257", _boundary_row(257)[None], True))
    for tag, rows_np, overflow in sets:
        lg = _bf16(rows_np).to(DEV)
        assert np.array_equal(lg.float().cpu().numpy(), rows_np)          # bf16-exact inputs
        n = rows_np.shape[0]
        for T, k, p in SR.PARAM_SETS + ((0.6, 4, 1.0),):
            keys = SH.entry_keys(rows_np, T)
            for pos0 in (0, 77):
                pos = [pos0 + r for r in range(n)]
                wflags = torch.zeros(1, dtype=torch.int32, device=DEV)
                wid, wu = sample(lg, T, k, p, DRAW_SEED, pos, want_u=True, flags=wflags)
                ref_ids, dec, ovf = SR.sample_rows(rows_np, T, k, p, DRAW_SEED, pos)
                assert bool(ovf.any()) == overflow and int(wflags.item()) == (4 if overflow else 0)
                assert (~dec | (wid.cpu().numpy() == ref_ids)).all()
                for parts in ([2048, 2048], [16, 4080]):
                    b = SH.bounds_of(parts)
                    for order, fin in (([0, 1], False), ([1, 0], False), ([1, 0], True)):
                        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
                        recs = []
                        ids, u = _chain(lg, b, order, (T, k, p), pos, None, flags, recs, finisher=fin)
                        assert torch.equal(ids, wid), (tag, T, k, p, parts, order, ids, wid)
                        assert torch.equal(u.view(torch.int32), wu.view(torch.int32))
                        assert int(flags.item()) == int(wflags.item()), (tag, T, k, p, parts, order)
                        for r in range(n):
                            want = SH.chain(keys[r], b, order, k)
                            for j in range(2):
                                assert np.array_equal(recs[j][r], want[j]), (tag, T, k, p, parts, order, r, j)
    # the all-equal row really is the mass-ties case in both shards of both cuts but the 16-column one
    assert (SR.crafted_rows(4096)[2] == 1.5).all()


def test_non_finite_rows_yield_in_range_ids():
    """NaN / +-inf logits have no defined draw (no bitwise claim); the chain still ends in columns
    inside the vocabulary and raises no error, and a finite row beside them is the whole head's."""
    from inferd_amd.runtime import sample
    lg = SR.bf16_logits(6, 1024).float()
    lg[0, :] = float("nan")
    lg[1, int(lg[1].argmax())] = float("nan")
    lg[2, 5] = float("inf")
    lg[3, 700:] = float("-inf")
    lg[4, :512] = float("nan")
    lgd = lg.to(torch.bfloat16).to(DEV)
    pos = [7, 8, 9, 10, 11, 12]
    for T, k, p in ((0.6, 20, 0.95), (1.0, 1, 1.0), (1.0, 64, 1.0)):
        wid = sample(lgd, T, k, p, DRAW_SEED, pos)
        for parts in ([512, 512], [16, 1008], [336, 16, 224, 448]):
            b = SH.bounds_of(parts)
            for order in _orders(len(parts)):
                ids, _ = _chain(lgd, b, order, (T, k, p), pos, None)
                got = ids.cpu().numpy()
                assert ((got >= 0) & (got < 1024)).all(), got
                assert got[5] == int(wid[5])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ span
LENS = (1, 17, 65)
SHARD_SETS = (((0, 384), (384, 640)), ((0, 16), (16, 1008)))


def _tiny(**kw):
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["tiny"]
    kw.setdefault("has_embed", False)
    kw.setdefault("has_lm_head", False)
    first, n = kw.pop("layers", (0, d.layers))
    s = SpanRuntime(d, first, n, device=DEV, kv_pages=16, max_tokens=256, max_seqs=4, max_positions=1024, **kw)
    s.init_synthetic(SEED)
    return s


def _span_chain(heads, order, nt, B, sampling, rs, pos, finisher=None):
    from inferd_amd.runtime import cand_record
    rec = None
    ids = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    for j, i in enumerate(order):
        last = j == len(order) - 1 and finisher is None
        new = cand_record(B, DEV)
        heads[i].head_shard_sampled(nt, B, sampling, rs, cand_in=rec, cand_out=new, positions=pos if last else None,
                                    ids=ids if last else None)
        rec = new
    if finisher is not None:
        finisher.head_shard_sampled(nt, B, sampling, rs, cand_in=rec, positions=pos, ids=ids)
    return ids


def test_span_shards_chain_equals_whole_head_span():
    """tiny model (vocab 1024): a whole-head span under set_sampling(row_seeds) free-runs a ragged
    prefill and 8 decode steps; a final_norm_out span fed the same ids hands its normed rows to lm_head
    shard spans (0,384),(384,640) and (0,16),(16,1008), chained in both orders, finished by the last
    shard or by a span owning no rows, and to the whole-head span's own head_shard_sampled: every
    chain's ids are the whole head's bit for bit; top_k = 1 gives the greedy head_shard ids."""
    from inferd_amd.runtime import row_seed_tensor
    params, B = (0.6, 20, 0.95), len(LENS)
    sampling = params + (DRAW_SEED,)
    rs_list = _row_seeds(B)
    rs = row_seed_tensor(rs_list, DEV)
    whole = _tiny(has_embed=True, has_lm_head=True)
    whole.set_sampling(*params, DRAW_SEED, row_seeds=rs_list)
    tail = _tiny(has_embed=True, final_norm_out=True)
    sets = [[_tiny(layers=(0, 0), head_first=f, head_rows=n) for f, n in ss] for ss in SHARD_SETS]
    norows = _tiny(layers=(0, 0))
    fresh = _tiny(has_embed=True, has_lm_head=True)          # a whole-head span that never sampled
    cur = torch.randint(0, 1024, (sum(LENS),), generator=torch.Generator().manual_seed(3))
    for step in range(9):
        reqs = [(f"s{i}", n if step == 0 else 1) for i, n in enumerate(LENS)]
        ow = whole.forward(reqs, ids=cur, want_hidden=False, want_next_ids=True)
        nt = tail.forward(reqs, ids=cur)["hidden"]
        pos = torch.tensor([n + step for n in LENS], dtype=torch.int32, device=DEV)
        want = ow["next_ids"]
        for heads in sets:
            for order in ([0, 1], [1, 0]):
                assert torch.equal(_span_chain(heads, order, nt, B, sampling, rs, pos), want), (step, order)
            assert torch.equal(_span_chain(heads, [1, 0], nt, B, sampling, rs, pos, finisher=norows), want), step
        assert torch.equal(_span_chain([fresh], [0], nt, B, sampling, rs, pos), want), step
        # top_k = 1: the greedy chain's ids
        gk, gids = None, torch.empty(B, dtype=torch.int32, device=DEV)
        for j, sp in enumerate(sets[0]):
            ko = torch.empty(B, dtype=torch.int64, device=DEV)
            sp.head_shard(nt, B, keys_in=gk, keys_out=ko, ids=gids if j == 1 else None)
            gk = ko
        # (top_p next to 0 removes everything behind the first kept entry, so that an exact tie of
        # two maximal logits -- which top_k = 1 keeps both of -- resolves to the lowest column as
        # argmax does, instead of by the draw)
        assert torch.equal(_span_chain(sets[0], [0, 1], nt, B, (1.0, 1, 1e-6, DRAW_SEED), rs, pos), gids), step
        cur = want
    for sp in [whole, fresh, norows] + sets[0] + sets[1]:
        sp.check_errors()


def test_span_refusals():
    sp = _tiny(layers=(0, 0), head_first=0, head_rows=384)
    nt = torch.zeros(16 * sp.dims.hidden, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="top_k"):
        sp.head_shard_sampled(nt, 2, (0.6, 0, 0.95, 1), cand_out=torch.zeros(2, 258, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="cand_out"):       # too small a record
        sp.head_shard_sampled(nt, 2, (0.6, 20, 0.95, 1), cand_out=torch.zeros(2, 100, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="required"):       # neither output
        sp.head_shard_sampled(nt, 2, (0.6, 20, 0.95, 1))
    with pytest.raises(RuntimeError, match="positions"):
        sp.head_shard_sampled(nt, 2, (0.6, 20, 0.95, 1), ids=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="lm_head"):          # unchanged: set_sampling needs the whole head
        sp.set_sampling(0.6, 20, 0.95, 1)


# ------------------------------------------------------------------ pipeline
# Ranks share cuda:0 and hand off over gloo (as tests/test_pipeline_gpu.py); every process that touches
# the GPU is a child with a time limit of its own, and a run stops at the first one that fails.
PIPE_SAMPLING = (0.6, 20, 0.95, 4242)
PB, PT, P_STEPS = 3, 20, 4
PIPE_SHARDS = {2: [(0, 512), (512, 512)], 3: [(0, 384), (384, 0), (384, 640)]}     # test_pipeline_gpu.HEAD_SHARDS
_REF = {}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _pipe_prompts(n_mb, vocab):
    g = torch.Generator().manual_seed(7)
    return [torch.randint(0, vocab, (PB, PT), generator=g) for _ in range(n_mb)]


def _pipe_worker(rank, world, port, sizes, n_mb, sharded, eager, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from inferd_amd.pipeline import PipelineStage
    from inferd_amd.runtime import MODELS
    d = MODELS["tiny"]
    first, n = sum(sizes[:rank]), sizes[rank]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = PipelineStage(d, rank, world, first, n, device=dev, seed=SEED, n_microbatches=n_mb, batch=PB,
                       max_ctx=PT + P_STEPS + 8, prefill_chunk=2, sharded_head=sharded, eager_decode=eager,
                       head_shard=PIPE_SHARDS[world][rank] if sharded else (0, 0), sampling=PIPE_SAMPLING)
    st.prefill(_pipe_prompts(n_mb, d.vocab))
    st.prepare_decode(P_STEPS)
    rec = []
    st.decode(2, record=rec)
    st.decode(P_STEPS - 2, record=rec)
    torch.cuda.synchronize()
    st.span.check_errors()
    if rank == 0:
        q.put([(k, m, t.cpu().tolist()) for k, m, t in rec])
    dist.barrier()
    st.release()
    dist.destroy_process_group()


def _ref_worker(n_mb, q):
    """one whole-head span under set_sampling, microbatch by microbatch: the prompt in the pipeline's
    prefill chunks (2 + 1 sequences), then a free run of P_STEPS - 1 decode steps"""
    from inferd_amd.runtime import MODELS, SpanRuntime
    d = MODELS["tiny"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sp = SpanRuntime(d, 0, d.layers, has_embed=True, has_lm_head=True, device=dev, kv_pages=2 * PB * n_mb + 4,
                     max_tokens=2 * (PT + P_STEPS + 8), max_seqs=PB, max_positions=PT + P_STEPS + 8)
    sp.init_synthetic(SEED)
    prompts = _pipe_prompts(n_mb, d.vocab)
    out = []
    for m in range(n_mb):
        seeds = [m * PB + b for b in range(PB)]
        parts = []
        for c in range(0, PB, 2):
            sp.set_sampling(*PIPE_SAMPLING, row_seeds=seeds[c:c + 2])
            ids = prompts[m][c:c + 2].reshape(-1).to(dev, torch.int32)
            parts.append(sp.forward([((m, b), PT) for b in range(c, min(c + 2, PB))], ids=ids, want_hidden=False,
                                    want_next_ids=True)["next_ids"])
        cur = torch.cat(parts)
        sp.set_sampling(*PIPE_SAMPLING, row_seeds=seeds)
        for k in range(P_STEPS):
            out.append((k, m, cur.cpu().tolist()))
            cur = sp.forward([((m, b), 1) for b in range(PB)], ids=cur, want_hidden=False, want_next_ids=True)["next_ids"]
    sp.check_errors()
    q.put(sorted(out))


def _collect(procs, q, timeout):
    """the queue's first item once every child has exited cleanly.  The children are watched while
    the result is awaited: a child that exits with an error (an exception in a rank, a GPU fault) fails
    the run at once -- the surviving ranks, blocked on their dead peer, are killed -- instead of the
    wait running into its time limit; nothing is left running either way."""
    import queue
    import time
    deadline = time.monotonic() + timeout
    rec = None
    try:
        while rec is None:
            try:
                rec = q.get(timeout=0.2)
            except queue.Empty:
                bad = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not bad, f"child process(es) exited with {bad} before a result arrived"
                assert time.monotonic() < deadline, f"no result within {timeout} s"
                if not any(p.is_alive() for p in procs):
                    rec = q.get(timeout=2)          # all exited cleanly: the result is in flight, or missing
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join()
    return rec


def _children(target, argsets, timeout=150):
    """run the child processes (each under the run's time limit) and return the queue's first item"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=a + (q,)) for a in argsets]
    for p in procs:
        p.start()
    return _collect(procs, q, timeout)


@pytest.mark.parametrize("eager", [True, False], ids=["eager", "graph"])
@pytest.mark.parametrize("sizes,n_mb,sharded", [([2, 2], 5, True), ([1, 1, 2], 7, True), ([2, 2], 5, False)],
                         ids=["2x2_vocab_head", "1-1-2_vocab_head", "2x2_whole_head"])
def test_pipeline_sampled_matches_whole_head_span(sizes, n_mb, sharded, eager):
    """PipelineStage(sampling=(0.6, 20, 0.95, seed)) with HIP spans, 4 steps: the vocab-parallel head
    (shards on every stage, one owning none) and the whole head on the last stage feed stage 0 exactly
    the ids of one whole-head span drawing under set_sampling with row seeds m * B + b, with eager
    decode steps and with replayed graphs."""
    world = len(sizes)
    if n_mb not in _REF:
        _REF[n_mb] = _children(_ref_worker, [(n_mb,)])
    port = _free_port()
    got = _children(_pipe_worker, [(r, world, port, sizes, n_mb, sharded, eager) for r in range(world)])
    assert len(got) == P_STEPS * n_mb
    assert sorted(got) == _REF[n_mb]
    by = {(k, m): ids for k, m, ids in got}
    assert any(by[(k, 0)] != by[(k, 1)] for k in range(P_STEPS))
