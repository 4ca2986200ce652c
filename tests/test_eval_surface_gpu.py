"""What _Trainer.test() leaves behind and main.report() prints, for every combination of the evaluation options: the set
of test_* attributes, every stored number against the same kernels called here on the same tensors, the returned list,
the report line, and that nothing reads a device value back while the loader is being consumed.  The net is a nearest
x4 upsampler, so only the bookkeeping is under test."""
import itertools
import types

import pytest
import torch

from oracle import fill
import lpips_ref
from test_niqe_gpu import _params_file

pytestmark = pytest.mark.gpu
SCALE = 4
NAN = float("nan")

# (LR size, target size, size of the third (bicubic) item or None)
ITEMS = (((25, 49), (100, 196), (100, 196)),     # every metric; NIQE at shave 2 sees 96 x 192: two blocks
         ((26, 74), (104, 296), (104, 296)),     # every metric; three blocks with remainders
         ((12, 10), (48, 40), None),             # fewer than two 96 x 96 blocks: no NIQE
         ((3, 4), (12, 16), None),               # under LPIPS's 16; at shave 2 under the 11 x 11 window
         ((2, 2), (8, 8), None),                 # PSNR only
         ((25, 49), (104, 200), (104, 200)))     # output and target differ: NIQE alone on the net's side, all four on the other
# which items count for which key, written from the table above
NET = {"psnr": (0, 1, 2, 3, 4), "ssim": (0, 1, 2, 3), "lpips": (0, 1, 2), "niqe": (0, 1, 5), "eval": (0, 1, 2)}
BICUBIC = {"psnr": (0, 1, 5), "ssim": (0, 1, 5), "lpips": (0, 1, 5), "niqe": (0, 1, 5)}
COMBOS = list(itertools.product((False, True), repeat=4))      # lpips, niqe, save_images, eval flags


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _items():
    out = []
    for i, (lr, hr, bc) in enumerate(ITEMS):
        item = [fill.rand((1, 3) + lr, 700 + i), fill.rand((1, 3) + hr, 720 + i)]
        if bc is not None:
            item.append(fill.rand((1, 3) + bc, 740 + i))
        out.append(tuple(item))
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_surface")
    _, _, _, vgg_sd, lin_sd = lpips_ref.filled_net()
    torch.save(vgg_sd, str(d / "vgg16.pth"))
    torch.save(lin_sd, str(d / "lins.pth"))
    return types.SimpleNamespace(vgg=str(d / "vgg16.pth"), lin=str(d / "lins.pth"), niqe=_params_file(d))


@pytest.fixture(scope="module")
def reference(gpu, files):
    """{(side, key, item): the number the kernels give for that picture}, computed once; 'niqe' per shave (0 and 2)."""
    pkg = _pkg()
    ops, utils = pkg.ops, pkg.utils
    net = pkg.models.LPIPS().load_vgg16(files.vgg).load_lins(files.lin).to(gpu).eval()
    params = utils.load_niqe_params(files.niqe)
    up = torch.nn.Upsample(scale_factor=SCALE, mode="nearest")
    ref = {}
    for i, item in enumerate(_items()):
        hr = item[1].to(gpu)
        sides = [("net", NET, up(item[0].to(gpu)))]
        if len(item) > 2:
            sides.append(("bicubic", BICUBIC, item[2].to(gpu)))
        for side, table, pic in sides:
            if i in table["psnr"]:
                ref[side, "psnr", i] = float(utils.PSNR(pic, hr))
            if i in table["ssim"]:
                ref[side, "ssim", i] = float(utils.SSIM(pic, hr))
            if i in table["lpips"]:
                with torch.no_grad():
                    ref[side, "lpips", i] = float(ops.lpips(pic.float(), hr.float(), net, normalize=True, reduce=True))
            if i in table["niqe"]:
                for shave in (0, 2):
                    ref[side, "niqe", shave, i] = ops.niqe(pic[0], params, shave)
            if i in table.get("eval", ()):
                s, p = ops.ssim(pic.float(), hr.float(), 2, "y8")[:2]
                ref[side, "eval", i] = (float(s), float(p))
    return ref


def _mean(v):
    return sum(v) / len(v)


def _expected(ref, lpips, niqe, save, ev):
    """The attributes test() must leave and their values, for one combination."""
    shave = 2 if ev else 0      # NIQE leaves out the border the eval row leaves out, else none

    def side(name, table):
        out = {"psnr": _mean([ref[name, "psnr", i] for i in table["psnr"]]),
               "ssim": _mean([ref[name, "ssim", i] for i in table["ssim"]])}
        if lpips:
            out["lpips"] = _mean([ref[name, "lpips", i] for i in table["lpips"]])
        if niqe:
            out["niqe"] = _mean([ref[name, "niqe", shave, i] for i in table["niqe"]])
        return out
    want = {"test_" + k: {"loader": v} for k, v in side("net", NET).items()}
    if save:
        want.update({"test_bicubic_" + k: {"loader": v} for k, v in side("bicubic", BICUBIC).items()})
    if ev:
        want["test_eval"] = {"loader": {"domain": "y8", "shave": 2,
                                        "psnr": _mean([ref["net", "eval", i][1] for i in NET["eval"]]),
                                        "ssim": _mean([ref["net", "eval", i][0] for i in NET["eval"]])}}
    return want


def _line(t, name, model, bicubic):
    """The report line of DESIGN.md section 36, formatted from the trainer's attributes."""
    def side(prefix):
        s = "PSNR %.4f SSIM %.4f" % (getattr(t, prefix + "psnr")[name], getattr(t, prefix + "ssim").get(name, NAN))
        if hasattr(t, "test_lpips"):
            s += " LPIPS %.4f" % getattr(t, prefix + "lpips").get(name, NAN)
        if hasattr(t, "test_niqe"):
            s += " NIQE %.4f" % getattr(t, prefix + "niqe").get(name, NAN)
        return s
    line = "%s: " % name
    if bicubic:
        line += "bicubic " + side("test_bicubic_") + ", "
    line += model + " " + side("test_")
    e = getattr(t, "test_eval", {}).get(name)
    if e:
        line += ", %s shave %d: PSNR %.4f SSIM %.4f" % (e["domain"], e["shave"], e["psnr"], e["ssim"])
    return line + "\n"


def _count_reads(monkeypatch):
    """Counts the calls that read a CUDA tensor back to the host."""
    counts = {}
    for name in ("cpu", "item", "tolist", "numpy", "__float__"):
        def wrapper(self, *a, _orig=getattr(torch.Tensor, name), _name=name, **kw):
            if self.is_cuda:
                counts[_name] = counts.get(_name, 0) + 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapper)
    return counts


@pytest.mark.parametrize("lpips,niqe,save,ev", COMBOS)
def test_attributes_numbers_report_and_no_read_back(gpu, files, reference, tmp_path, monkeypatch, capsys, lpips, niqe, save, ev):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    pkg = _pkg()
    argv = ["--model_name", "EDSR", "--num_channels", "3", "--scale_factor", str(SCALE), "--synthetic", "--save_dir", str(tmp_path)]
    if lpips:
        argv += ["--lpips_vgg", files.vgg, "--lpips_lin", files.lin]
    if niqe:
        argv += ["--niqe_params", files.niqe]
    args = cli.parse_args(argv)
    t = TRAINERS["EDSR"](args)
    t.model = torch.nn.Upsample(scale_factor=SCALE, mode="nearest").to(t.device)
    before = set(vars(t))
    items = _items()
    counts = _count_reads(monkeypatch)
    marks = []

    def loader():
        marks.append(dict(counts))
        for item in items:
            yield item
        marks.append(dict(counts))
    kw = dict(eval_shave=2, eval_domain="y8") if ev else {}
    got = t.test(loader(), save_images=save, **kw)
    monkeypatch.undo()
    assert len(marks) == 2
    if save:      # utils.save_img copies every picture to the host: the counters do see such a call
        assert marks[1].get("cpu", 0) - marks[0].get("cpu", 0) >= len(items), marks
    else:
        assert marks[0] == marks[1], marks

    want = _expected(reference, lpips, niqe, save, ev)
    have = {a for a in set(vars(t)) - before if a.startswith("test_")}
    assert have == set(want)
    for attr in sorted(want):
        assert getattr(t, attr) == want[attr], attr
    up = t.model
    psnr = [float(pkg.utils.PSNR(up(lr.to(gpu)), hr.to(gpu))) for lr, hr in (item[:2] for item in items[:5])]
    assert got == psnr and all(type(v) is float for v in got)

    capsys.readouterr()
    for test_only, save_flag in ((True, False), (True, True), (False, False)):
        if save_flag and not save:
            continue        # --save_test_images runs test(save_images=True): there is no such report after a plain test()
        args.test_only, args.save_test_images = test_only, save_flag
        cli.report(t, args)
        out = capsys.readouterr().out
        if test_only or ev:
            assert out == _line(t, "loader", "EDSR", save_flag)
        else:
            assert out == ""
