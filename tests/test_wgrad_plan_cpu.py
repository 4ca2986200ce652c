"""The case table of tests/test_wgrad_bf_gpu.py against the library's weight-gradient planner (csrc/conv_wgrad_plan.h,
asked through srk_conv2d_backward_weight_plan), for the 256 CUs of an MI355X.  Runs anywhere: the query is host arithmetic.

The GPU test asserts srk_last_kernel_name() per row, so a row that drifted off its branch fails there too -- but only
on a GPU.  Here the drift shows on every machine, together with which variants the table as a whole still reaches."""
import itertools

import pytest

import __graft_entry__
import wgrad_plan_ref as R


@pytest.fixture(scope="module", autouse=True)
def _built():
    __graft_entry__.build()


# every k_wgrad_bf variant the table must reach (what srk_last_kernel_name() reports, "k_wgrad_bf<...>")
REQUIRED = {
    "4,1,2,spec", "4,1,2,spec,pf,ring", "4,1,2,spec,scalar", "4,1,2,spec,grouped", "4,1,2,tile,scalar",
    "4,1,1,spec", "4,1,1,spec,pf,ring", "4,1,1,spec,scalar", "4,1,1,spec,grouped", "4,1,1,spec,pf,ring,grouped",
    "4,1,1,spec,scalar,grouped", "4,1,1,tile,scalar",
    "2,2,2,spec,pf,ring", "2,2,2,spec,scalar", "2,2,2,spec,pf,ring,grouped", "2,2,2,tile",
}


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
def test_case_lands_in_its_variant(c):
    p = R.plan_case(c)
    assert p is not None and p.name == c.name, (c.row, p)
    for key, val in c.want.items():
        if key == "idle":
            assert (p.idle_blocks > 0) == val, (c.row, p)
        else:
            assert getattr(p, key) == val, (c.row, key, p)
    assert p.kernel == "bf"        # never k_wgrad_tr: that kernel has its own tests
    # the K loop a row is named for: K33 is the 3x3 one, everything else runs the generic loop
    if c.row <= 32:
        assert p.spec and c.N >= 2
        # N is the smallest batch that plans as spec: one image fewer is the per-tile variant
        q = R.plan(c.N - 1, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.pad, dy_ps_r=c.ps, n=c.n, x_aligned=not p.scalar,
                   dy_aligned=not p.scalar)
        assert not q.spec, (c.row, q)
    else:
        assert not p.spec
    # what the plan says must be consistent with what the staging mode of the name means
    assert p.ring == p.prefetch or not p.spec
    if p.scalar:
        assert not p.prefetch


def test_table_reaches_every_required_variant():
    reached = {R.plan_case(c).name[len("k_wgrad_bf<"):-1] for c in R.CASES}
    assert reached == REQUIRED, (sorted(reached - REQUIRED), sorted(REQUIRED - reached))
    # and, inside the spec variants, both K loops with and without the ring, both dY layouts
    facts = {(R.plan_case(c).ring, (c.kh, c.kw) == (3, 3), c.ps > 1) for c in R.CASES if R.plan_case(c).spec}
    for ring in (False, True):
        for k33 in (False, True):
            assert (ring, k33, False) in facts
        assert (ring, True, True) in facts
    # idle ring blocks, swizzled grids in spec and tile, 1 .. 3 input-channel chunks, two output-channel blocks
    plans = [R.plan_case(c) for c in R.CASES]
    assert any(p.idle_blocks for p in plans) and any(p.swizzle and p.spec for p in plans)
    assert any(p.swizzle and not p.spec for p in plans)
    assert {p.gy for p in plans} >= {1, 2, 3} and {p.gz for p in plans} >= {1, 2}
    assert any(p.HH == p.TH and p.ring for p in plans)       # 1x1: no halo rows, the ring advances by all its rows


def test_no_plannable_tile_prefetches_without_the_ring():
    """conv_wgrad_plan.h asserts at compile time that every tile inside the LDS budget has room for the ring and for two
    buffer sets; here the planner is asked over a grid of problems that reaches every tile height and width it can
    choose: no plan has `prefetch && !ring`, and wb_split's LDS clause never decides."""
    plans = 0
    widths = (1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48)
    for cout, k, OH, OW in itertools.product((64, 32, 16), (1, 2, 3), range(1, 18), widths):
        p = R.plan(64, OH + k - 1, OW + k - 1, 64, cout, k, k, 0)
        assert p is not None, (cout, k, OH, OW)
        plans += 1
        assert not (p.prefetch and not p.ring), (cout, k, OH, OW, p)
        assert 2 * p.lds + 8 * 1024 <= 160 * 1024, (cout, k, OH, OW, p)
    assert plans == 1836


def test_idle_ring_blocks_formula():
    """ntiles just above 2 G: blocks take ceil(ntiles / G) consecutive tiles, so a third of them get none"""
    p = R.plan_case(R.BY_ID["one_tile_row"])
    assert (p.ntiles, p.G, p.idle_blocks) == (515, 256, 84)
    per = R.cdiv(p.ntiles, p.G)
    assert per == 3 and sum(1 for b in range(p.G) if b * per < p.ntiles) == p.G - p.idle_blocks
