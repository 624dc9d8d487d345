"""PipelineStage(sharded_head=True, sampling=...) on CPU ranks over gloo: the candidate record of the
sampled vocab-parallel head handed round the ring.

Each rank runs its span with an oracle executor whose sampled head is the numpy reference of the
record and the merge (tests/sampling_shard_ref.py), so the test checks the schedule: the record's
place in the head record, which shard starts it, the positions and row seeds the finishing call
draws with.  Every id fed to stage 0 must equal a single-span oracle run that draws with
sampling_ref.sample_rows under the same seed, row seeds (m * B + b) and positions."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sampling_ref as SR
import sampling_shard_ref as SH
import test_pipeline_gloo as G
from oracle import qwen3_ref as R

SEED = G.SEED
SAMPLING = (0.6, 20, 0.95, 777)
B, T_PROMPT = 3, 9


def _logits(x, lm):
    """bf16 logits of normed rows x [rows, h] over lm rows [n, h], accumulated in fp64 so that a logit
    does not depend on the shard (the slice of lm) that computes it -- the engine's GEMV property"""
    return (x.double() @ lm.double().T).float().to(torch.bfloat16).float().numpy()


class SampledOracleExecutor(G.OracleExecutor):
    """OracleExecutor plus the sampled head's interface (SpanExecutor.set_sampling / head_sampled)"""

    def set_sampling(self, sampling, row_seeds):
        self.sampling, self.row_seeds = sampling, row_seeds
        self.steps = {}

    def prefill(self, sessions, n_tokens, ids=None, x=None, want_ids=False):
        self.prompt_len = n_tokens
        return super().prefill(sessions, n_tokens, ids=ids, x=x, want_ids=want_ids)

    def decode(self, m):
        super().decode(m)
        self.steps[m] = self.steps.get(m, 0) + 1

    def head_sampled(self, normed, rows, m, cand_in=None, cand_out=None, ids=None, positions=None):
        from inferd_amd.pipeline import unpack_rows
        T, k, p, seed = self.sampling
        recs = [None] * rows if cand_in is None else list(cand_in.numpy().view(np.uint64).reshape(rows, SH.WORDS))
        if self.lm is not None:
            lg = _logits(unpack_rows(normed.reshape(-1), rows, self.dims.hidden), self.lm)
            keys = SH.entry_keys(lg, T, first_col=self.head_first)
            recs = [SH.fold(recs[r], keys[r], 0, keys.shape[1], k) for r in range(rows)]
        if cand_out is not None:
            cand_out.copy_(torch.from_numpy(np.stack(recs).view(np.int64)).reshape(cand_out.shape))
        if ids is not None:
            # the device ctx_lens of the microbatch after its last decode step: the drawn token's position
            pos = [self.prompt_len + self.steps.get(m, 0)] * rows if positions is None else positions.tolist()
            for r in range(rows):
                d = SH.dist_of_record(recs[r], self.dims.vocab, p)
                ids[r] = d.draw(SR.uniform(seed, int(self.row_seeds[m][r]), int(pos[r])))[0]


def _prompts(n_mb, vocab, twin):
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, vocab, (B, T_PROMPT), generator=g) for _ in range(n_mb)]
    if twin:
        prompts[1] = prompts[0].clone()        # equal prompts in two microbatches
    return prompts


def _worker(rank, world, port, n_steps, q, n_mb):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from inferd_amd.pipeline import PipelineStage
    d = R.CONFIGS["tiny"]
    rg = G._split(d, world, None)[rank]
    head = G.HEAD_SHARDS[world][rank]
    ex = SampledOracleExecutor(d, rg, rank == 0, rank == world - 1, True, head)
    st = PipelineStage(d, rank, world, rg.first_layer, rg.n_layers, device="cpu", seed=SEED, n_microbatches=n_mb,
                       batch=B, max_ctx=64, prefill_chunk=2, executor=ex, sharded_head=True, head_shard=head,
                       sampling=SAMPLING, **rg.span_kwargs())
    assert st.head_rec[0].numel() == st.normed_bytes + 8 * B * SH.WORDS
    st.prefill(_prompts(n_mb, d.vocab, True))
    st.prepare_decode(n_steps)
    rec = []
    st.decode(2, record=rec)
    st.decode(n_steps - 2, record=rec)
    if rank == 0:
        q.put([(k, m, t.tolist()) for k, m, t in rec] + [("final", m, st.ids[m].tolist()) for m in range(n_mb)])
    dist.barrier()
    dist.destroy_process_group()


def _reference(n_mb, n_steps):
    """one span over all layers ending in the final norm, its own whole lm_head, sampling_ref's draw"""
    d = R.CONFIGS["tiny"]
    sp = R.RefSpan(d, SEED, 0, d.layers - 1, True, False, torch.bfloat16, "sdpa", final_norm_out=True)
    lm = R.gen_global_weights(d, SEED)["lm_head"]
    T, k, p, seed = SAMPLING
    prompts = _prompts(n_mb, d.vocab, True)

    def draw(normed_row, m, b, pos):
        lg = _logits(normed_row.reshape(1, -1).to(torch.bfloat16), lm)
        ids, _, ovf = SR.sample_rows(lg, T, k, p, seed, [pos], [m * B + b])
        assert not ovf.any()
        return int(ids[0])
    feeds = {}
    for m in range(n_mb):
        for b in range(B):
            nxt = draw(sp.forward_cached((m, b), prompts[m][b:b + 1])[0, -1], m, b, T_PROMPT)
            for s in range(n_steps + 1):
                feeds[(s, m, b)] = nxt
                nxt = draw(sp.forward_cached((m, b), torch.tensor([[nxt]]))[0, -1], m, b, T_PROMPT + s + 1)
    return feeds


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


def _run_ring(world, n_steps, n_mb):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = G._free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_steps, q, n_mb)) for r in range(world)]
    for p in procs:
        p.start()
    return _collect(procs, q, 300)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sampled_vocab_parallel_ring_matches_single_span(world):
    """worlds 2, 3 (the middle stage owns no lm_head rows) and 4 (the first stage owns none), n_mb =
    2S + 1: every (step, microbatch) fed to stage 0 is the single span's draw; two microbatches with
    equal prompts draw differently somewhere (distinct row seeds)."""
    n_steps, n_mb = 4, 2 * world + 1
    rec = _run_ring(world, n_steps, n_mb)
    ref = _reference(n_mb, n_steps)
    G._check(rec, ref, n_steps, n_mb)
    fed = {(k, m): ids for k, m, ids in rec}
    assert any(fed[(k, 0)] != fed[(k, 1)] for k in list(range(n_steps)) + ["final"])


def test_sampling_parameters_are_validated():
    from inferd_amd.pipeline import PipelineStage
    d = R.CONFIGS["tiny"]
    with pytest.raises(ValueError, match="top_k"):
        PipelineStage(d, 0, 1, 0, d.layers, device="cpu", seed=SEED, n_microbatches=1, batch=B, max_ctx=64,
                      executor=object(), sampling=(0.6, 0, 0.95, 1))
