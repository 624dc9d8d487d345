"""CPU tests of the sampled vocab-parallel head: the exactness of the candidate-record merge
(tests/sampling_shard_ref.py) against the whole row's reference (tests/sampling_ref.py) for every
partition and chain order the GPU tests use, and the host surface of the new calls (C-ABI exports,
argument validation without a GPU, torch op schemas, the ABI version)."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import sampling_ref as SR
import sampling_shard_ref as SH


def _orders(n, tag):
    sh = list(range(n))
    random.Random(f"{tag}/{n}").shuffle(sh)
    if sh == list(range(n)):
        sh = sh[::-1]
    return list(range(n)), sh


def _check_rows(rows_np, params, cut_list, tag):
    """every row, parameter set, cut and chain order: the chained record's kept list, overflow and
    top-p distribution are the whole row's"""
    checked = 0
    for T, k, p in params:
        keys = SH.entry_keys(rows_np, T)
        for r in range(rows_np.shape[0]):
            d = SR.RowDist(rows_np[r], T, k, p)
            for parts in cut_list:
                b = SH.bounds_of(parts)
                for order in _orders(len(parts), tag):
                    rec = SH.chain(keys[r], b, order, k)[-1]
                    kept, ovf = SH.finish(rec)
                    assert np.array_equal(kept, d.order) and ovf == d.overflow, (tag, T, k, p, r, parts, order)
                    checked += 1
            # top-p on the record = top-p on the row (one cut is enough: the record is the same)
            dr = SH.dist_of_record(rec, rows_np.shape[1], p)
            assert np.array_equal(dr.kept, d.kept) and dr.overflow == d.overflow
            assert np.array_equal(dr.cum, d.cum)
    return checked


@pytest.mark.parametrize("vocab", [48, 1024, 151936])
def test_merge_is_exact_on_the_gpu_tests_inputs(vocab):
    lg = SR.bf16_logits(64, vocab).float().numpy()
    n = _check_rows(lg, SR.PARAM_SETS, SH.cuts(vocab), f"randn{vocab}")
    assert n == 64 * len(SR.PARAM_SETS) * len(SH.cuts(vocab)) * 2


def test_merge_is_exact_on_crafted_rows():
    """ties straddling the k-th value, all-equal logits (capacity overflow), maxima in the first /
    last tile; the cuts of the GPU test included"""
    rows = SR.crafted_rows(4096)
    cut_list = SH.cuts(4096) + [[2048, 2048], [16, 4080]]
    _check_rows(rows, SR.PARAM_SETS + ((0.6, 4, 1.0),), cut_list, "crafted4096")
    d = SR.RowDist(rows[2], 0.6, 20, 0.95)
    assert d.overflow                                       # the all-equal row does overflow


def boundary_row(n_equal, vocab=4096):
    """n_equal columns at 1.5 (spread over both halves and the first tile), the rest far below"""
    row = np.full(vocab, -8.0, dtype=np.float32)
    first = n_equal // 2
    row[np.arange(first) * 3 % 2048] = 1.5                  # 128 distinct columns < 2048 (3 is odd)
    row[2048 + np.arange(n_equal - first) * 5 % 2048] = 1.5
    assert int((row == 1.5).sum()) == n_equal
    return row


@pytest.mark.parametrize("n_equal,flag", [(256, False), (257, True)])
def test_overflow_flag_is_exact_at_the_capacity_boundary(n_equal, flag):
    """exactly 256 / 257 qualifying columns, split 128 / 128(+1) and [16, rest]: clear at 256, set at 257"""
    row = boundary_row(n_equal)
    d = SR.RowDist(row, 0.6, 20, 0.95)
    assert d.overflow == flag and d.n_topk == 256
    keys = SH.entry_keys(row, 0.6)
    for parts in ([2048, 2048], [16, 4080]):
        b = SH.bounds_of(parts)
        if parts[0] == 2048:
            assert int((row[:2048] == 1.5).sum()) == 128 and int((row[2048:] == 1.5).sum()) == n_equal - 128
        for order in ([0, 1], [1, 0]):
            kept, ovf = SH.finish(SH.chain(keys, b, order, 20)[-1])
            assert ovf == flag and np.array_equal(kept, d.order), (parts, order)


def test_record_of_a_short_shard_holds_all_its_columns():
    """a shard with fewer than top_k columns contributes all of them; an empty shard passes the record on"""
    row = SR.bf16_logits(1, 1024).float().numpy()[0]
    keys = SH.entry_keys(row, 1.0)
    rec = SH.shard_record(keys, 0, 16, 64)
    assert int(rec[0]) == 16 and sorted(SH.entry_col(SH.entries_of(rec)).tolist()) == list(range(16))
    assert np.array_equal(SH.entry_s(SH.entries_of(rec)), np.sort(row[:16])[::-1])
    assert np.array_equal(SH.fold(rec, keys, 16, 16, 64), rec)


# ------------------------------------------------------------------ host surface
NEW = ("inferd_sample_cand_bytes", "inferd_span_head_shard_sampled", "inferd_sample_shard")


def test_new_symbols_exported_and_bound():
    from inferd_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.load().inferd_abi_version() == _lib.ABI_VERSION == 5       # additions within ABI 5
    assert _lib.SAMPLE_CAND_ENTRIES == SH.ENTRIES == 257
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "inferd_span.h")).read()
    assert "#define INFERD_SAMPLE_CAND_ENTRIES 257" in hdr


def test_cand_bytes():
    from inferd_amd import _lib
    lib = _lib.load()
    for rows in range(1, 65):
        assert lib.inferd_sample_cand_bytes(rows) == rows * SH.WORDS * 8 > 0
    assert lib.inferd_sample_cand_bytes(0) == -1 and lib.inferd_sample_cand_bytes(65) == -1
    assert lib.inferd_sample_cand_bytes(16) == 33024                       # ~33 KB per hop at B = 16


@pytest.mark.parametrize("T,k,p,word", [(0.0, 20, 0.95, "temperature"), (float("nan"), 20, 0.95, "temperature"),
                                        (0.6, 0, 0.95, "top_k"), (0.6, 65, 0.95, "top_k"), (0.6, 20, 0.0, "top_p"),
                                        (0.6, 20, 1.5, "top_p")])
def test_bad_parameters_fail_before_any_device_call(T, k, p, word):
    from inferd_amd import _lib
    lib = _lib.load()
    sp = _lib.Sampling(temperature=T, top_k=k, top_p=p, seed=1, row_seeds=None)
    buf = (ctypes.c_int64 * 1024)()
    a = ctypes.addressof(buf)
    assert lib.inferd_sample_shard(a, 1, 16, 0, sp, None, a, a, a, None, None, None) == _lib.INFERD_ERR_ARG
    assert word.encode() in lib.inferd_last_error()
    # the span call checks the parameters before it looks at the span
    assert lib.inferd_span_head_shard_sampled(None, a, 1, sp, None, a, a, a, None, None, None) == _lib.INFERD_ERR_ARG
    assert word.encode() in lib.inferd_last_error()


def test_bad_arguments_are_refused():
    from inferd_amd import _lib
    lib = _lib.load()
    sp = _lib.Sampling(temperature=0.6, top_k=20, top_p=0.95, seed=1, row_seeds=None)
    buf = (ctypes.c_int64 * 1024)()
    a = ctypes.addressof(buf)
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a += a % 16                                             # 16-byte aligned
    ERR = _lib.INFERD_ERR_ARG

    def shard(logits=a, rows=1, cols=16, first=0, cin=None, cout=a, pos=a, ids=a):
        rc = lib.inferd_sample_shard(logits, rows, cols, first, sp, cin, cout, pos, ids, None, None, None)
        return rc, lib.inferd_last_error()

    for kw, word in (({"rows": 0}, b"rows"), ({"rows": 65}, b"rows"), ({"cols": 24}, b"cols"), ({"cols": -16}, b"cols"),
                     ({"cols": 16 * 24576 + 16}, b"cols"), ({"first": 8}, b"first_col"), ({"first": -16}, b"first_col"),
                     ({"logits": None}, b"logits"), ({"logits": a + 8}, b"aligned"), ({"cout": None, "ids": None}, b"required"),
                     ({"pos": None}, b"positions"), ({"cin": a + 4}, b"aligned"), ({"cout": a + 4}, b"aligned")):
        rc, msg = shard(**kw)
        assert rc == ERR and word in msg, (kw, msg)
    assert lib.inferd_sample_shard(a, 1, 16, 0, None, None, a, a, a, None, None, None) == ERR
    # the span call: null parameters, null span, missing outputs
    assert lib.inferd_span_head_shard_sampled(None, a, 1, None, None, a, a, a, None, None, None) == ERR
    assert lib.inferd_span_head_shard_sampled(None, a, 1, sp, None, a, a, a, None, None, None) == ERR
    assert b"head_shard_sampled" in lib.inferd_last_error()
    # set_sampling keeps refusing what it refused
    assert lib.inferd_span_set_sampling(None, sp) == ERR and b"null span" in lib.inferd_last_error()


def test_torch_ops_registered():
    import inferd_amd.ops as O
    for name in ("span_head_shard_sampled", "sample_shard", "sample_cand_bytes"):
        assert name in O.OPS and hasattr(torch.ops.inferd, name)
    assert str(torch.ops.inferd.sample_cand_bytes.default._schema) == "inferd::sample_cand_bytes(int rows) -> int"
    assert str(torch.ops.inferd.span_head_shard_sampled.default._schema) == \
        "inferd::span_head_shard_sampled(int span, Tensor normed, int rows, float temperature, int top_k, " \
        "float top_p, int seed, Tensor? row_seeds, Tensor? cand_in, Tensor(a!)? cand_out, Tensor? positions, " \
        "Tensor(b!)? ids, Tensor(c!)? u_out=None, Tensor(d!)? logits=None) -> ()"
    assert str(torch.ops.inferd.sample_shard.default._schema) == \
        "inferd::sample_shard(Tensor? logits, int rows, int first_col, float temperature, int top_k, float top_p, " \
        "int seed, Tensor? row_seeds, Tensor? cand_in, Tensor(a!)? cand_out, Tensor? positions, Tensor(b!)? ids, " \
        "Tensor(c!)? u_out=None, Tensor(d!)? flags=None) -> ()"
    assert torch.ops.inferd.sample_cand_bytes(16) == 33024
    with pytest.raises(RuntimeError, match="rows"):
        torch.ops.inferd.sample_cand_bytes(65)
