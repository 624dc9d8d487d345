"""CPU tests of sampled decoding: the numpy reference of the draw (tests/sampling_ref.py) against
transformers' warpers, the counter generator's uniformity, the share of undecidable cases on the
GPU tests' inputs, and the host surface (C-ABI exports, parameter validation without a GPU, torch
op schemas, the ABI version)."""
import ctypes

import numpy as np
import pytest
import torch

import sampling_ref as SR

SEED = 20240607
POSITIONS = (0, 1, 2, 63, 64, 2047, 8191, 40959)


def _hf_kept(l_f32: np.ndarray, T, k, p):
    """the columns transformers' warpers leave finite, as client.py:95-101 chains them"""
    from transformers import LogitsProcessorList, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    procs = LogitsProcessorList([TemperatureLogitsWarper(float(T)), TopKLogitsWarper(int(k)), TopPLogitsWarper(float(p))])
    out = procs(torch.zeros((1, 1), dtype=torch.long), torch.from_numpy(l_f32.copy())[None])
    return set(torch.nonzero(torch.isfinite(out[0])).reshape(-1).tolist())


def test_reference_kept_set_matches_transformers():
    """Temperature, top-k (ties at the k-th value kept) and top-p of the reference leave the columns
    transformers' TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper leave, on every row
    whose top-p cut is decidable and does not fall between two equal values (transformers orders
    equal values by its sort, the engine by column).  Rows with planted ties across the k-th value
    included."""
    lg = SR.bf16_logits(16, 1024).float().numpy()
    planted = SR.crafted_rows(1024, k=20)[[1, 3, 4]]
    planted64 = SR.crafted_rows(1024, k=64)[[1]]
    rows = np.concatenate([lg, planted, planted64])
    compared, tie_sets = 0, 0
    for T, k, p in SR.PARAM_SETS:
        for r in range(rows.shape[0]):
            d = SR.RowDist(rows[r], T, k, p)
            if not d.cut_decidable:
                continue
            m = d.kept.size
            if m < d.n_topk and d.sk[m - 1] == d.sk[m]:      # the cut splits a group of equal values
                continue
            assert set(d.kept.tolist()) == _hf_kept(rows[r], T, k, p), (T, k, p, r)
            compared += 1
            tie_sets += d.n_topk > min(k, 1024)
    assert compared >= 0.9 * len(SR.PARAM_SETS) * rows.shape[0]
    assert tie_sets >= 4          # kept sets larger than k were among them


def test_counter_generator_is_uniform():
    """20,000 positions on one fixed 1024-column row, (1.0, 20, 1.0): every kept token's frequency
    within 5 sigma of its probability."""
    row = SR.bf16_logits(1, 1024, gen_seed=5).float().numpy()[0]
    d = SR.RowDist(row, 1.0, 20, 1.0)
    n = 20000
    wg = SR.wg
    key = SR._sm(SR._sm(SEED) + 3)
    with np.errstate(over="ignore"):
        x = wg.splitmix64(np.uint64(key) + np.arange(n, dtype=np.uint64))
    u = ((x >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    assert float(u[17]) == float(SR.uniform(SEED, 3, 17)) and u.min() >= 0.0 and u.max() < 1.0
    idx = np.minimum(np.searchsorted(d.cum, u.astype(np.float64), side="right"), d.kept.size - 1)
    counts = np.bincount(idx, minlength=d.kept.size)
    sigma = np.sqrt(n * d.probs * (1 - d.probs))
    z = np.abs(counts - n * d.probs) / np.maximum(sigma, 1e-9)
    assert z.max() < 5.0, z.max()


@pytest.mark.parametrize("vocab", [48, 1024, 151936])
def test_undecidable_share_is_capped(vocab):
    """On the GPU tests' inputs (64 rows of randn * 3 in bf16, 8 positions, the four parameter sets)
    at most 5 % of the cases are undecidable, so the exact comparison cannot hide a failure."""
    lg = SR.bf16_logits(64, vocab).float().numpy()
    pos = np.array([[p] * 64 for p in POSITIONS])
    sizes = set()
    for T, k, p in SR.PARAM_SETS:
        ids, dec, ovf = SR.sample_rows(lg, T, k, p, SEED, pos)
        assert dec.mean() >= 0.95, (T, k, p, dec.mean())
        assert not ovf.any()
        sizes |= {SR.RowDist(lg[r], T, k, p).n_topk for r in range(0, 64, 7)}
    if vocab > 48:
        assert min(sizes) == 1 and max(sizes) > 64        # kept sets from 1 to beyond k: ties happen


def test_reference_capacity_rule():
    """All-equal logits at V = 4096: the first 256 columns are kept, overflow is reported, and
    top-p 0.95 leaves 244 of them."""
    row = SR.crafted_rows(4096)[2]
    d = SR.RowDist(row, 0.6, 20, 0.95)
    assert d.overflow and d.n_topk == 256 and d.kept.tolist() == list(range(244))


def test_sampling_symbols_exported_and_bound():
    from inferd_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("inferd_sample", "inferd_span_set_sampling"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.Sampling) == 32 and _lib.Sampling.seed.offset == 16
    assert _lib.load().inferd_abi_version() == 5        # additions within ABI 5


@pytest.mark.parametrize("T,k,p,word", [(0.0, 20, 0.95, "temperature"), (-1.0, 20, 0.95, "temperature"),
                                        (float("nan"), 20, 0.95, "temperature"), (0.6, 0, 0.95, "top_k"),
                                        (0.6, 65, 0.95, "top_k"), (0.6, 20, 0.0, "top_p"), (0.6, 20, 1.5, "top_p")])
def test_bad_parameters_fail_before_any_device_call(T, k, p, word):
    """rc 1 (INFERD_ERR_ARG) with a message through ctypes, on a machine without a GPU; the Python
    wrappers raise ValueError."""
    from inferd_amd import _lib
    from inferd_amd.runtime import check_sampling_params
    lib = _lib.load()
    sp = _lib.Sampling(temperature=T, top_k=k, top_p=p, seed=1, row_seeds=None)
    buf = (ctypes.c_int32 * 64)()
    assert lib.inferd_sample(ctypes.addressof(buf), 1, 16, sp, ctypes.addressof(buf), ctypes.addressof(buf), None, None,
                             None) == _lib.INFERD_ERR_ARG
    assert word.encode() in lib.inferd_last_error()
    assert lib.inferd_span_set_sampling(None, sp) == _lib.INFERD_ERR_ARG
    assert word.encode() in lib.inferd_last_error()
    with pytest.raises(ValueError, match=word):
        check_sampling_params(T, k, p)


def test_good_parameters_reach_the_argument_checks():
    from inferd_amd import _lib
    lib = _lib.load()
    sp = _lib.Sampling(temperature=0.6, top_k=20, top_p=0.95, seed=1, row_seeds=None)
    assert lib.inferd_span_set_sampling(None, sp) == _lib.INFERD_ERR_ARG and b"null span" in lib.inferd_last_error()
    assert lib.inferd_sample(None, 1, 16, sp, None, None, None, None, None) == _lib.INFERD_ERR_ARG
    assert b"required" in lib.inferd_last_error()
    buf = (ctypes.c_int32 * 64)()
    a = ctypes.addressof(buf)
    for rows, vocab in ((0, 16), (65, 16), (1, 24), (1, 16 * 24576 + 16)):
        assert lib.inferd_sample(a, rows, vocab, sp, a, a, None, None, None) == _lib.INFERD_ERR_ARG


def test_sampling_torch_ops_registered():
    import inferd_amd.ops as O
    assert "span_set_sampling" in O.OPS and "sample" in O.OPS
    assert str(torch.ops.inferd.span_set_sampling.default._schema) == \
        "inferd::span_set_sampling(int span, float temperature, int top_k, float top_p, int seed, " \
        "Tensor? row_seeds, bool on) -> ()"
    assert str(torch.ops.inferd.sample.default._schema) == \
        "inferd::sample(Tensor logits, float temperature, int top_k, float top_p, int seed, Tensor? row_seeds, " \
        "Tensor positions, Tensor(a!) ids, Tensor(b!)? u_out, Tensor(c!)? flags) -> ()"


def test_session_row_seed_is_stable():
    """The row seed of a session is a fixed function of its id (not Python's salted hash)."""
    import hashlib
    from inferd_amd.partitioned_models import session_row_seed
    assert session_row_seed(None) == 0
    want = int.from_bytes(hashlib.blake2b(b"chat-17", digest_size=8).digest(), "little")
    assert session_row_seed("chat-17") == want and 0 <= want < 2 ** 64
    assert session_row_seed("chat-18") != want
