"""The case table of the stride-1 convolution epilogue tests (tests/stride1_epilogue_ref.py), checked without a GPU: these
are conditions on the INPUTS, so that a pass of tests/test_stride1_epilogue_gpu.py means something.

Coverage: every (family, option it accepts) and every (family, option that makes it decline) pair of FAMILIES has a row --
the declining rows on the family the layer falls to.  Attainable bars: torch's fp32 CPU convolution with the same
epilogue stays within HALF of every row's bar of the float64 reference, so a row that misses its bar on the device cannot
blame the inputs.  Activations that discriminate: 25 .. 75 % of the pre-activations (mask sources) are negative, and
tanh / sigmoid rows keep 90 % of them inside |z| < 3, where a wrong value is not squashed.  Residuals that do not hide
the convolution: rms(residual or add_to) <= 2 rms(convolution term), because the bar's atol is rtol * rms(reference)."""
import numpy as np
import pytest
import torch

import stride1_epilogue_ref as R
from conftest import TOL_TIGHT, assert_close_elementwise
from conv_abi import _ratio

assert R.TOL_TIGHT == TOL_TIGHT
IDS = [c.id for c in R.CASES]


def test_ids_are_unique_and_rows_are_well_formed():
    assert len(R.BY_ID) == len(R.CASES)
    for c in R.CASES:
        assert c.kind in ("fwd", "dgrad") and c.tol in (R.TOL_BF, R.TOL_TIGHT), c.id
        assert set(c.epi) <= set("bRlpPtsnr234AZN" if c.kind == "fwd" else "mza24X"), c.id
        assert R.family(c) == "refused" or R.family(c) in R.FAMILIES, c.id
        r = R.ps_r(c)
        if r:
            assert c.cout % (r * r) == 0 and (c.kind == "fwd" or (c.cout // (r * r)) % 8 == 0), c.id
        assert not ("A" in c.epi and "Z" in c.epi), c.id
        if "n" in c.epi:
            assert R.act(c) in ("prelu1", "preluC"), c.id
        if c.decl:
            fam, opt = c.decl.split(":")
            assert opt in R.FAMILIES[fam]["declines"] and R.family(c) in R.FAMILIES[fam]["declines"][opt], c.id
            known = {o for f in R.FAMILIES.values() for o in f["accepts"]} | {"cout_mod16"}
            if opt in known:      # (the option is one options() can see: the row must really have it)
                have = R.options(c)
                assert opt in have | {R.DECL_ALIAS.get(o, o) for o in have}, (c.id, opt, have)


@pytest.mark.parametrize("fam", sorted(R.FAMILIES))
def test_every_family_option_pair_has_a_row(fam):
    spec = R.FAMILIES[fam]
    rows = [c for c in R.CASES if R.family(c) == fam]
    assert rows or not spec["accepts"], "no row runs %s" % fam
    for opt in spec["accepts"]:
        assert any(opt in R.options(c) for c in rows), "%s accepts %s: no row" % (fam, opt)
    for opt, falls_to in spec["declines"].items():
        hit = [c for c in R.CASES if c.decl == "%s:%s" % (fam, opt)]
        assert hit, "%s declines %s: no row" % (fam, opt)
        assert {R.family(c) for c in hit} == set(falls_to), (fam, opt, [c.id for c in hit])


def test_vocabulary_of_the_issue_is_present():
    """pixel shuffle 2 / 3 / 4 with runs that are and (r = 2, 3) are not a multiple of 4; per-channel PReLU behind one; one
    prelu1 and one preluC row with a negative slope; y_amax given and not; x_nchw"""
    fwd = [c for c in R.CASES if c.kind == "fwd"]
    for r in (2, 3, 4):
        assert any(R.ps_r(c) == r and "ps_vec" in R.options(c) for c in fwd), r
    for r in (2, 3):
        assert any(R.ps_r(c) == r and "ps_ragged" in R.options(c) and "r" in c.epi for c in fwd), r
    assert any("preluC_ps" in R.options(c) for c in fwd)
    assert any("n" in c.epi and R.act(c) == "prelu1" for c in fwd) and any("n" in c.epi and R.act(c) == "preluC" for c in fwd)
    assert any("A" in c.epi for c in fwd) and any("Z" in c.epi for c in fwd) and any("N" in c.epi for c in fwd)
    assert any("A" not in c.epi and "Z" not in c.epi for c in fwd)
    # N = 2 on two ragged tiles, with a residual, in every family that runs (the batch stride of y and of the residual)
    for fam in R.FAMILIES:
        rows = [c for c in R.CASES if R.family(c) == fam]
        assert not rows or any(c.N >= 2 and c.H >= 9 and ("r" in c.epi or "a" in c.epi or fam in ("rowsw", "rowsr", "bfw", "tapk",
                                                                                                  "tapkm")) for c in rows), fam
    for fam in ("tapk", "tapkm"):
        assert any(R.family(c) == fam and c.N >= 2 and "a" in c.epi for c in R.CASES), fam
    for o in ("b", "r", "y", "x"):
        assert any(R.off(c, o) == 4 for c in fwd), o


@pytest.mark.parametrize("cid", IDS)
def test_inputs_make_a_pass_meaningful(cid):
    c = R.BY_ID[cid]
    ref = R.reference(cid)
    out64 = ref["out"].numpy()
    # the bar is attainable: plain fp32 arithmetic uses at most half of it
    out32 = R.compute(cid, torch.float32)["out"].numpy()
    used = _ratio(out32, out64, c.tol)
    assert used <= 0.5, "%s: fp32 on the CPU uses %.3f of the bar %.0e" % (cid, used, c.tol)
    assert_close_elementwise(out32, out64, c.tol, what=cid)
    # the activation / the mask decides both ways
    if ref["pre"] is not None:
        z = ref["pre"].numpy()
        neg = float((z < 0).mean())
        assert 0.25 <= neg <= 0.75, "%s: %.2f of the pre-activations are negative" % (cid, neg)
        if R.act(c) in ("tanh", "sigmoid"):
            inside = float((np.abs(z) < 3).mean())
            assert inside >= 0.9, "%s: only %.2f of the pre-activations inside |z| < 3" % (cid, inside)
    # the addend does not hide the convolution
    if ("r" in c.epi and c.kind == "fwd") or "a" in c.epi:
        rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
        res, term = R.tensors(cid)["res"].numpy(), ref["term"].numpy()
        assert rms(res) <= 2.0 * rms(term), "%s: rms(addend) %.3g against rms(conv term) %.3g" % (cid, rms(res), rms(term))
