"""Data prep: vocabulary on the host, co-occurrence on the GPU, checked against the
fixtures produced by the reference's own `src/data/text8.py` (tests/golden/make_text8_golden.py)."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import glove_ref as ref

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = [("cov90_ctx5", 0.9, 5), ("cov100_ctx2", 0.999, 2)]


@pytest.mark.parametrize("tag,coverage,context", CASES)
def test_vocabulary_matches_reference(tag, coverage, context):
    from trainer import text8
    tokens = (GOLDEN / "text8_corpus.txt").read_text().split()
    vocab, counts, props = text8.create_vocabulary(tokens, None, coverage)
    want = pd.read_csv(GOLDEN / ("text8_%s_vocab.csv" % tag), keep_default_na=False, na_filter=False)
    assert list(counts) == list(want["count"])                       # same cutoff, same <UNK> mass
    np.testing.assert_allclose(props, want["proportion"].astype(float), rtol=1e-15)
    # same tokens; the order may only differ inside groups of equal count (pandas' unstable sort, text8.py:80)
    assert sorted(vocab) == sorted(want["token"])
    for c in np.unique(counts):
        assert set(np.asarray(vocab, object)[counts == c]) == set(want["token"][want["count"] == c])
    ids = text8.token_ids(tokens, vocab)
    assert ids.dtype == np.int32 and ids.min() >= 0 and ids.max() < len(vocab)


@pytest.mark.gpu
@pytest.mark.parametrize("n,V,context", [(0, 5, 3), (1, 5, 3), (50, 4, 1), (5000, 60, 5), (20000, 1000, 5),
                                         (3000, 7, 9), (200000, 50000, 5)])
def test_cooccurrence_kernel_vs_oracle(hip, n, V, context):
    import torch
    rng = np.random.default_rng(n + V)
    p = 1.0 / np.arange(1, V + 1)
    tok = rng.choice(V, size=n, p=p / p.sum()).astype(np.int32)
    row, col, cnt, val = hip.cooccurrence(torch.from_numpy(tok).cuda(), V, context)
    if n == 0:
        assert row.numel() == 0
        return
    w_row, w_col, w_cnt, w_val = ref.cooccurrence(tok, context)
    np.testing.assert_array_equal(row.cpu().numpy(), w_row)            # integer work: bit-exact
    np.testing.assert_array_equal(col.cpu().numpy(), w_col)
    np.testing.assert_array_equal(cnt.cpu().numpy(), w_cnt)
    np.testing.assert_allclose(val.cpu().numpy(), w_val, rtol=1e-12)
    assert (row != col).all()


@pytest.mark.gpu
@pytest.mark.parametrize("tag,coverage,context", CASES)
def test_prep_end_to_end_matches_reference_files(hip, tag, coverage, context, tmp_path):
    """corpus -> vocab.txt + interaction.csv, compared with the files the reference module wrote."""
    from trainer import text8
    from trainer.data_utils import load_interaction_csv
    corpus = (GOLDEN / "text8_corpus.txt").read_text()
    want_vocab = (GOLDEN / ("text8_%s_vocab.txt" % tag)).read_text().split("\n")
    data = text8.process_data(corpus, None, coverage, context, hip=hip, seed=3)
    # pin the id assignment to the reference's (ties inside equal counts are its unstable sort's choice)
    remap = np.asarray([want_vocab.index(t) for t in data["vocabulary"][0]])
    text8.save_data(data, tmp_path)
    got = pd.read_csv(tmp_path / "interaction.csv", keep_default_na=False, na_filter=False)
    want = pd.read_csv(GOLDEN / ("text8_%s_interaction.csv" % tag), keep_default_na=False, na_filter=False)
    assert list(got.columns) == list(want.columns)
    got["row_token_id"], got["col_token_id"] = remap[got["row_token_id"]], remap[got["col_token_id"]]
    got = got.sort_values(["row_token_id", "col_token_id"]).reset_index(drop=True)
    assert len(got) == len(want)
    for c in ("row_token_id", "col_token_id", "count", "row_token", "col_token"):
        assert (got[c].astype(str) == want[c].astype(str)).all(), c
    for c in ("value", "neg_weight", "glove_weight", "glove_value"):
        np.testing.assert_allclose(got[c].astype(float), want[c].astype(float), rtol=1e-12, err_msg=c)
    # and the trainer's loader accepts the files as written
    coo = load_interaction_csv(str(tmp_path / "interaction.csv"), str(tmp_path / "vocab.txt"))
    assert len(coo["row"]) == len(want) and coo["row"].max() < len(want_vocab)
    assert (tmp_path / "vocab.csv").exists()


# ---- the edges of glove_cooccurrence_i32: cap overflow, sentinel-only input, the widest window, keys with high bits
GUARD = 64
PATTERNS = {"row": -7, "col": -8, "cnt": -9, "val": -1.5}


def cooccurrence_raw(hip, tok, V, context, cap):
    """glove_cooccurrence_i32 itself (GloveHip.cooccurrence raises where nnz exceeds cap): (rc, nnz, outputs), every output
    cap + GUARD long and filled with a pattern beforehand."""
    import torch
    from trainer.hip_api import _stream
    tokens = torch.from_numpy(np.ascontiguousarray(tok, np.int32)).cuda()
    out = {"row": torch.full((cap + GUARD,), PATTERNS["row"], dtype=torch.int32, device="cuda:0"),
           "col": torch.full((cap + GUARD,), PATTERNS["col"], dtype=torch.int32, device="cuda:0"),
           "cnt": torch.full((cap + GUARD,), PATTERNS["cnt"], dtype=torch.int64, device="cuda:0"),
           "val": torch.full((cap + GUARD,), PATTERNS["val"], dtype=torch.float64, device="cuda:0")}
    nnz = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(max(hip.lib.glove_cooc_workspace_bytes(len(tok), context), 256), dtype=torch.uint8, device="cuda:0")
    rc = hip.lib.glove_cooccurrence_i32(tokens.data_ptr(), len(tok), V, context, out["row"].data_ptr(), out["col"].data_ptr(),
                                        out["cnt"].data_ptr(), out["val"].data_ptr(), nnz.data_ptr(), cap, ws.data_ptr(),
                                        ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc, int(nnz.item()), {k: v.cpu().numpy() for k, v in out.items()}


def assert_equals_oracle(got, want, m):
    """The first m entries of the outputs against the oracle's first m (integers bit-exact, values rtol 1e-12)."""
    w_row, w_col, w_cnt, w_val = want
    np.testing.assert_array_equal(got["row"][:m], w_row[:m])
    np.testing.assert_array_equal(got["col"][:m], w_col[:m])
    np.testing.assert_array_equal(got["cnt"][:m], w_cnt[:m])
    np.testing.assert_allclose(got["val"][:m], w_val[:m], rtol=1e-12)


def zipf_tokens(n, V):
    rng = np.random.default_rng(n + V)
    p = 1.0 / np.arange(1, V + 1)
    return rng.choice(V, size=n, p=p / p.sum()).astype(np.int32)


@pytest.mark.gpu
def test_cooccurrence_cap_overflow_reports_the_true_size_and_writes_cap_entries(hip):
    import torch
    from trainer.hip_api import GloveHipError
    n, V, context = 5000, 60, 5
    tok = zipf_tokens(n, V)
    want = ref.cooccurrence(tok, context)
    true_nnz = len(want[0])
    assert true_nnz > 100
    for cap in (true_nnz, true_nnz - 1, true_nnz // 2, 0):
        rc, nnz, got = cooccurrence_raw(hip, tok, V, context, cap)
        assert rc == 0 and nnz == true_nnz, cap              # *out_nnz: the true size, beyond cap too
        assert_equals_oracle(got, want, cap)                 # the first cap entries are the oracle's first cap
        for name, pattern in PATTERNS.items():               # nothing behind cap was written
            assert (got[name][cap:] == pattern).all(), (cap, name)
    for cap in (true_nnz - 1, true_nnz // 2, 0):
        with pytest.raises(GloveHipError):
            hip.cooccurrence(torch.from_numpy(tok).cuda(), V, context, cap=cap)
    row, _, _, _ = hip.cooccurrence(torch.from_numpy(tok).cuda(), V, context, cap=true_nnz)      # an exact fit is none
    assert row.numel() == true_nnz


@pytest.mark.gpu
def test_cooccurrence_of_inputs_that_emit_only_sentinel_keys(hip):
    import torch
    for tok, context in ((np.full(1000, 3, np.int32), 5), (np.array([4, 4], np.int32), 3), (np.array([2], np.int32), 255)):
        assert len(ref.cooccurrence(tok, context)[0]) == 0
        rc, nnz, got = cooccurrence_raw(hip, tok, 7, context, 16)
        assert rc == 0 and nnz == 0
        for name, pattern in PATTERNS.items():
            assert (got[name] == pattern).all()
        assert all(t.numel() == 0 for t in hip.cooccurrence(torch.from_numpy(tok).cuda(), 7, context))
    # fewer tokens than the window, all distinct: every pair of positions is one entry each way
    tok, context = np.array([5, 1, 6, 2], np.int32), 5
    want = ref.cooccurrence(tok, context)
    rc, nnz, got = cooccurrence_raw(hip, tok, 7, context, 32)
    assert rc == 0 and nnz == len(want[0]) == 12
    assert_equals_oracle(got, want, nnz)
    assert (got["row"][nnz:] == PATTERNS["row"]).all()


@pytest.mark.gpu
def test_cooccurrence_at_the_widest_window(hip):
    n, V, context = 600, 40, 255
    tok = zipf_tokens(n, V)
    want = ref.cooccurrence(tok, context)
    rc, nnz, got = cooccurrence_raw(hip, tok, V, context, V * V)
    assert rc == 0 and nnz == len(want[0])
    assert_equals_oracle(got, want, nnz)
    assert cooccurrence_raw(hip, tok, V, 256, V * V)[0] == -1                # GLOVE_E_BADARG: a key holds offsets up to 255
    assert cooccurrence_raw(hip, tok, V, 256, V * V)[1] == -1                # ... and *out_nnz was not touched


@pytest.mark.gpu
def test_cooccurrence_keys_that_use_their_upper_bits(hip):
    """V = 1.3e9, context 5: V V context = 8.45e18, just under the 9.0e18 guard; the keys of the ids next to V - 1 need 63
    bits.  The oracle's int64 keys (a V + b) stay below 2^63 here."""
    V, context, n = 1_300_000_000, 5, 5000
    assert float(V) * V * context < 9.0e18 and (V - 1) * V + (V - 1) < 2 ** 63 and ((V - 1) * V + V - 1) * context + 4 > 2 ** 62
    rng = np.random.default_rng(11)
    ids = np.concatenate([[V - 1], V - 1 - rng.choice(np.arange(1, 11), 5, replace=False), [0, 1, 65535, 65536, 2 ** 30, 2 ** 30 + 1]])
    tok = rng.choice(ids, n).astype(np.int32)
    assert tok.min() >= 0 and len(np.unique(tok)) == len(np.unique(ids))
    want = ref.cooccurrence(tok, context)
    rc, nnz, got = cooccurrence_raw(hip, tok, V, context, 256)
    assert rc == 0 and nnz == len(want[0]) and nnz > 100
    assert_equals_oracle(got, want, nnz)
    assert got["row"][:nnz].max() == V - 1 and got["col"][:nnz].max() == V - 1
    assert cooccurrence_raw(hip, tok, 1_400_000_000, context, 256)[:2] == (-1, -1)      # 9.8e18: refused, nothing written
