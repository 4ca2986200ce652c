"""The phase decomposition of strided TRANS gathers (csrc/conv_tile.h: what for_each_phase launches from, asked of the
library through tests/strided_phase_ref.py) without a GPU: a transposed convolution computed phase by phase in float64
numpy -- every output element written exactly once into a NaN-filled tensor -- against
torch.nn.functional.conv_transpose{1,2}d, over every geometry of a small grid; and the declared edges of the GPU table
against the library's phases.

The sweeps' sizes are asserted, so they cannot shrink without notice:
  1-D  stride 1..4, kernel 1..9, padding 0..k-1, output padding 0..s-1, input 1..7:  2871 problems with a non-empty
       output, 351 zero-tap phases, 166 problems that skip at least one phase
  2-D  KH != KW on a thinned grid, stride 2..4:  530 problems, 1181 zero-tap phases, 114 problems that skip a phase"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__
import strided_phase_ref as R


@pytest.fixture(scope="module", autouse=True)
def _built():
    __graft_entry__.build()


def _deconv_1d_by_phase(x, w, s, p, O):
    """x [I], w [K] -> (out [O] NaN where nothing was written, writes per element, zero-tap phases, phases run)"""
    out = np.full(O, np.nan)
    writes = np.zeros(O, dtype=np.int64)
    zero = 0
    ph = R.phases_1d(len(w), s, p, O)
    for o0, P, Kv, i0, w0, wd in ph:
        zero += Kv == 0
        for r in range(P):
            acc = 0.0
            for u in range(Kv):
                i = r + i0 + u
                if 0 <= i < len(x):
                    acc += x[i] * w[w0 + wd * u]
            out[o0 + r * s] = acc
            writes[o0 + r * s] += 1
    return out, writes, zero, len(ph)


def test_phases_1d_exhaustive():
    rs = np.random.RandomState(11)
    problems = zero_tap = skipping = 0
    for s, k in itertools.product(range(1, 5), range(1, 10)):
        w = rs.standard_normal(k)
        for p, op, H in itertools.product(range(k), range(s), range(1, 8)):
            O = R.out_dim(H, k, s, p, 1, op)
            if O <= 0:
                continue
            x = rs.standard_normal(H)
            out, writes, zero, nph = _deconv_1d_by_phase(x, w, s, p, O)
            assert (writes == 1).all(), (s, k, p, op, H)
            ref = F.conv_transpose1d(torch.from_numpy(x)[None, None], torch.from_numpy(w)[None, None], None, s, p, op)[0, 0]
            assert ref.shape[0] == O
            assert np.abs(out - ref.numpy()).max() <= 1e-12, (s, k, p, op, H)
            problems += 1
            zero_tap += zero
            skipping += nph < s
    assert (problems, zero_tap, skipping) == (2871, 351, 166)


def _deconv_2d_by_phase(x, w, s, p, OH, OW):
    """x [IH, IW], w [KH, KW] -> (out, writes, zero-tap phases, phases run)"""
    IH, IW = x.shape
    out = np.full((OH, OW), np.nan)
    writes = np.zeros((OH, OW), dtype=np.int64)
    ph = R.phases(w.shape[0], w.shape[1], s, p, OH, OW)
    for q in ph:
        for r in range(q.PH):
            for c in range(q.PW):
                acc = 0.0
                for u in range(q.KHv):
                    for v in range(q.KWv):
                        iy, ix = r + q.iy0 + u, c + q.ix0 + v
                        if 0 <= iy < IH and 0 <= ix < IW:
                            acc += x[iy, ix] * w[q.wh0 + q.wdh * u, q.ww0 + q.wdw * v]
                out[q.oy0 + r * s, q.ox0 + c * s] = acc
                writes[q.oy0 + r * s, q.ox0 + c * s] += 1
    return out, writes, sum(q.KHv * q.KWv == 0 for q in ph), len(ph)


SWEEP_2D = (530, 1181, 114)       # problems, zero-tap phases, problems that skip a phase
GRID_2D = [(s, kh, kw) for s in (2, 3, 4) for kh, kw in ((1, 2), (2, 5), (3, 1), (3, 5), (4, 9), (5, 3), (9, 4))]


def test_phases_2d_rectangular_kernels():
    rs = np.random.RandomState(12)
    problems = zero_tap = skipping = 0
    for s, kh, kw in GRID_2D:
        w = rs.standard_normal((kh, kw))
        for p, op, (H, W) in itertools.product((0, 1, 2), (0, s - 1), ((1, 1), (1, 5), (2, 3), (4, 1), (5, 4))):
            OH, OW = R.out_dim(H, kh, s, p, 1, op), R.out_dim(W, kw, s, p, 1, op)
            if OH <= 0 or OW <= 0:
                continue
            x = rs.standard_normal((H, W))
            out, writes, zero, nph = _deconv_2d_by_phase(x, w, s, p, OH, OW)
            assert (writes == 1).all(), (s, kh, kw, p, op, H, W)
            ref = F.conv_transpose2d(torch.from_numpy(x)[None, None], torch.from_numpy(w)[None, None], None, s, p, op)[0, 0]
            assert tuple(ref.shape) == (OH, OW)
            assert np.abs(out - ref.numpy()).max() <= 1e-12, (s, kh, kw, p, op, H, W)
            problems += 1
            zero_tap += zero
            skipping += nph < s * s
    assert (problems, zero_tap, skipping) == SWEEP_2D


def test_phases_is_the_product_of_its_axes():
    for s, kh, kw, p, OH, OW in itertools.product((1, 2, 3, 4), (1, 3, 4), (2, 5, 9), (0, 1, 3), (1, 2, 7), (1, 5, 6)):
        want = [R.Phase(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], a[5], b[4], b[5])
                if a[2] and b[2] else R.Phase(a[0], b[0], a[1], b[1], 0, 0, 0, 0, 0, 0, 0, 0)
                for a in R.phases_1d(kh, s, p, OH) for b in R.phases_1d(kw, s, p, OW)]
        assert R.phases(kh, kw, s, p, OH, OW) == want


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
def test_table_rows_have_the_edges_they_claim(c):
    OH, OW = R.dims(c)
    assert OH > 0 and OW > 0
    assert 1 <= c.N <= 3 and all(1 <= v <= 40 for v in (c.H, c.W)), "shapes stay small"
    assert c.props == R.properties(c), (sorted(c.props), sorted(R.properties(c)))
    if c.exact == "zero_tap":
        assert "zero_tap" in c.props and c.kind == "fwd"
    if c.exact == "dead":
        assert c.kind == "dgrad" and c.props & {"zero_tap", "dead_rows"}
        assert any(any(row) for row in R.untouched(c))
    if "multi_tile" in c.props and c.kind != "wgrad":
        # ragged: the phase is no whole number of blocks either
        trans, IH, IW, IC, GH, GW, OC = R.gather(c)
        sizes = [q.PH * q.PW for q in R.case_phases(c)] if trans else [GH * GW]
        assert any(n > c.block and n % c.block for n in sizes)


def test_table_covers_what_it_is_for():
    fwd = [c for c in R.CASES if c.kind == "fwd"]
    have = lambda prefix, prop: any(c.prefix.startswith(prefix) and prop in c.props for c in R.CASES)
    for prefix in ("k_conv_bfd_mp<", "k_conv_bfd<1,1,", "k_conv_bfd<2,2,2,", "k_conv_bf3<", "k_conv_tapn<", "k_conv_mfma<",
                   "k_gather_conv"):
        assert have(prefix, "zero_tap"), prefix
    for prefix in ("k_conv_bfd_mp<", "k_conv_bfd<1,1,", "k_conv_bfd<1,4,", "k_conv_bfd<2,4,", "k_conv_bfd<3,4,",
                   "k_conv_bfd<4,4,", "k_conv_bfd<2,2,2,", "k_conv_bf3<", "k_conv_tapn<", "k_conv_direct<", "k_conv_mfma<"):
        assert have(prefix, "multi_tile"), prefix
    assert have("k_conv_bfd<1,1,", "skipped") and have("k_conv_bfd<1,4,", "skipped") and have("k_gather_conv", "skipped")
    assert {c.prefix[:len("k_conv_bfd<1,1,1")] for c in fwd if c.prefix.startswith("k_conv_bfd<1,1,")} == \
        {"k_conv_bfd<1,1,%d" % now for now in (1, 2, 3, 4)}
    assert sum(c.algo == "f16x3" for c in fwd) == 2 and sum(c.algo == "bf16x6" and "SRK_BFD_SMALL" in dict(c.env) for c in fwd) == 2
    # the phase count in k_conv_bfd_mp's name is the library's
    for c in R.CASES:
        if c.prefix.startswith("k_conv_bfd_mp<") and c.prefix.endswith("x4"):
            assert len(R.case_phases(c)) == 4, c.id
