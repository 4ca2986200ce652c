"""Train-step bodies of the reference's trainers on the MI355X path.

A train step is a list of SEGMENTS, [(fn(*batch) -> out, dp or None), ...]: the step
    zero_grad -> forward -> loss -> backward -> [RCCL all-reduce] -> [clip] -> optimizer step
cut behind every backward pass whose gradients a DataParallel has to exchange.  `eager_step(segments)` is the closure
step(*batch) -> device loss tensor(s) that runs them in order (an exchange after each segment with a dp); every `*_step`
builder returns such a closure, with the same op order, loss and hyper-parameters as the cited reference lines and with
NO host synchronisation (the reference syncs every iteration through loss.data[0], edsr.py:158).  `GraphedSegments`
captures the same segments as hipGraphs -- one graph on a single GPU, graphs split at the exchanges under data
parallelism -- so the eager, the one-graph and the split-graph form of a step are one definition.  `GraphedFn` (any
function, one graph), `GraphedStep` (a loss step) and `capture_step` (any eager step) are its callers.
"""
import contextlib
import gc

import torch

from . import ops
from .layers import bump_weight_epoch
from .optim import FlatParams, make_optimizer


@contextlib.contextmanager
def _no_gc_during_capture():
    """hipGraph objects must not be destroyed while a stream is capturing (`hipErrorStreamCaptureUnsupported`, raised
    from a destructor = process abort).  An earlier GraphedStep / GraphedSegments that is only reachable through a
    reference cycle (bound methods in its segment list) is freed by the cyclic garbage collector at an arbitrary
    allocation — e.g. in the middle of the next capture.  Collect first, keep the collector off while capturing."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()
        quiesce_gc()     # (what the capture built stays for the life of the step)


def quiesce_gc():
    """Take the cyclic collector out of the steady-state step.  A process that has imported torch tracks ~170 k container
    objects; one automatic full (generation-2) collection walks all of them: 73 - 83 ms measured (tools/dp_step_times.py),
    landing inside whichever train step crosses the threshold -- the 83 ms step among 1.6 ms ones of round 5's driver run,
    and under data parallelism a straggler every other rank waits for.  After set-up (model, optimizer, captured graphs)
    everything alive is long-lived: collect once, then gc.freeze() moves it to the permanent generation, so later
    collections only look at what a step allocates (< 1 ms).  Reference counting still frees frozen objects."""
    gc.collect()
    gc.freeze()


def _static_buffers(example_inputs):
    """Static input buffers of a captured step.  4-D image batches are kept channels_last: the copy of a new batch into
    the buffer (one strided copy either way) then delivers the layout the first convolution reads, and the captured step
    holds no layout kernel."""
    out = []
    for t in example_inputs:
        if t.dim() == 4 and t.is_floating_point():
            out.append(torch.empty_like(t, memory_format=torch.channels_last).copy_(t))
        else:
            out.append(torch.empty_like(t).copy_(t))
    return out


def _active(dp):
    return dp is not None and dp.active


def _backward(loss, dp):
    """loss.backward() of the reference (edsr.py:154 ...) for one loss or a list of losses (lapsrn.py:196-197: several
    backward calls into the same gradients).  Single GPU: the deferred weight gradients are launched (grouped) when the
    autograd engine finishes the pass.  Data parallel: they stay pending so that dp.exchange() can interleave the grouped
    launches with the gradient buckets; the backward is seeded with 1/world."""
    # (premasked_gradients: a train step reads parameter gradients only, so activation gradients may travel pre-masked)
    if _active(dp):
        with ops.manual_wgrad_flush(), ops.premasked_gradients():
            ops.backward(loss, dp.loss_seed)
    else:
        with ops.premasked_gradients():
            ops.backward(loss)   # seeded with the persistent ones tensor: no fill, no scale pass (ops.unit_seed)
        ops.flush_wgrads()  # (weight gradients recorded outside an engine callback)


def _seeded(dp):
    """Context for computing a loss that `_backward(loss, dp)` will seed: under data parallelism the 1/world seed is
    folded into the loss gradient by the loss kernel itself (ops.loss_seed)."""
    if _active(dp):
        return ops.loss_seed(1.0 / dp.world, dp.loss_seed)
    return contextlib.nullcontext()


def eager_step(segments):
    """The eager form of a step given as segments: every fn in order, dp.exchange() behind a segment that has a dp (the
    weight gradients its backward left pending and the all-reduce; without an active dp a no-op flush).  Returns what
    the last fn returned.  `step.segments` keeps the definition, so a captured form is built from the closure alone."""
    def step(*batch):
        out = None
        for fn, dp in segments:
            out = fn(*batch)
            if dp is not None:
                dp.exchange()
        return out
    step.segments = segments
    return step


def loss_segments(model, opt, loss_fn, dp=None, clip=None):
    """The plain loss step, loss_fn(model(input), *targets), cut at its gradient exchange:
    [(zero_grad + seeded loss + backward, dp), ([clip] + optimizer step, None)]."""
    out = []

    def fwd_bwd(inp, *targets):
        opt.zero_grad()
        with _seeded(dp):
            loss = loss_fn(model(inp), *targets)
        _backward(loss, dp)
        out.append(loss)
        return loss

    def update(*batch):
        if clip is not None:
            opt.clip_grad_norm(clip)
        opt.step()
        return out.pop()

    return [(fwd_bwd, dp), (update, None)]


def mixed_loss(pixel, ssim_weight=0.0, fft_weight=0.0, fft_norm="backward", lpips_weight=0.0, lpips_net=None):
    """The loss a kind trains on: `pixel` itself (the same function object) for all weights 0, else
    [(1 - a) * pixel(pred, t) + a * (1 - SSIM(pred, t))] + w * FFT(pred, t) + v * LPIPS(pred, t): the mix of Zhao et al.
    (a = ssim_weight), the frequency-domain L1 of ops.fft_loss (w = fft_weight >= 0) and ops.lpips with lpips_net (v =
    lpips_weight >= 0; models.LPIPS; every kind's batches are in [0, 1], so normalize=True), added by srk_axpby
    (ops.loss_sum); on one GPU each loss kernel folds its weight into its gradient (ops.weighted_term), so each extra term
    adds its loss launches, the axpby of two scalars and the axpby of two gradients to a step, and no ATen node to a
    captured one.  A term whose weight is 0 leaves the result the object it is without that term."""
    a, w, v = float(ssim_weight), float(fft_weight), float(lpips_weight)
    if not 0.0 <= v < float("inf"):
        raise ValueError("lpips_weight %r is not a non-negative finite number" % (lpips_weight,))
    if v > 0.0 and lpips_net is None:
        raise ValueError("lpips_weight %r needs an lpips_net (models.LPIPS with its weights loaded)" % (lpips_weight,))
    if not 0.0 <= a <= 1.0:
        raise ValueError("ssim_weight %r is not in [0, 1]" % (ssim_weight,))
    if not 0.0 <= w < float("inf"):
        raise ValueError("fft_weight %r is not a non-negative finite number" % (fft_weight,))
    if fft_norm not in ops.FFT_NORMS:
        raise ValueError("fft_norm %r is not one of %s" % (fft_norm, ops.FFT_NORMS))
    if a == 0.0:
        base = pixel
    else:
        def base(pred, target):
            p1, p2 = ops.fork(pred)   # the two gradients of pred are added by srk_axpby, not by autograd's ATen add
            return ops.loss_sum(ops.weighted_term(pixel, 1.0 - a, p1, target), ops.weighted_term(ops.ssim_loss, a, p2, target),
                                1.0 - a, a)

    def stage(inner, fn, weight):
        def loss(pred, target):
            p1, p2 = ops.fork(pred)
            # (inner carries weight 1: its terms take their own weights, or the general path, exactly as without this term)
            return ops.loss_sum(inner(p1, target), ops.weighted_term(fn, weight, p2, target), 1.0, weight)
        return loss
    # the additive terms, innermost first; a new one is one more pair here (and a flag in sr_trainers.TERM_FLAGS)
    for weight, fn in ((w, lambda pred, t: ops.fft_loss(pred, t, fft_norm)),
                       (v, lambda pred, t: ops.lpips(pred, t, lpips_net, normalize=True))):
        if weight > 0.0:
            base = stage(base, fn, weight)
    return base


def mse_step(model, opt, dp=None, clip=None, **terms):
    """srcnn.py:127-131 / fsrcnn.py:153-157 / vdsr.py:143-150 (clip = 0.4).  terms: mixed_loss's keywords."""
    return eager_step(loss_segments(model, opt, mixed_loss(ops.mse_loss, **terms), dp, clip))


def l1_step(model, opt, dp=None, **terms):
    """edsr.py:151-155.  terms: mixed_loss's keywords."""
    return eager_step(loss_segments(model, opt, mixed_loss(ops.l1_loss, **terms), dp))


def lapsrn_step(model, opt, dp=None, **terms):
    """lapsrn.py:190-199: two Charbonnier losses, two backward calls into the same gradients.  A plain closure without
    segments: it cannot be split at its exchange, so under data parallelism it is never captured."""
    loss_fn = mixed_loss(ops.charbonnier_loss, **terms)   # both levels

    def step(inp, target2x, target4x):
        opt.zero_grad()
        hr2, hr4 = model(inp)
        with _seeded(dp):
            l1 = loss_fn(hr2, target2x)
            l2 = loss_fn(hr4, target4x)
        _backward([l1, l2], dp)
        if dp is not None:
            dp.exchange()
        opt.step()
        return l1, l2
    return step


def vespcn_segments(model, opt, mc_weight=0.01, flow_weight=0.001, dp=None):
    """VESPCN's joint step (Caballero et al. 2017, eq. 7) on frames [B,3,C,H,W] and the shaved centre HR frame:
      loss = MSE(sr, hr) + mc_weight * mc + flow_weight * flow_huber(total flow),
    mc the motion-compensation loss of ops.motion_fuse and the flow the MotionCompensator's, in pixels, for both
    neighbours.  On one GPU each weight in (0, 1) is declared as its term's seed (ops.loss_seed, as ops.weighted_term
    does), so the two kernels fold it into the gradient they write and no scale pass runs; the sums are srk_axpby
    (ops.loss_sum).  The same cut as loss_segments: [(zero_grad + forward + loss + backward, dp), (optimizer step, None)]."""
    mc_weight, flow_weight = float(mc_weight), float(flow_weight)
    for name, v in (("mc_weight", mc_weight), ("flow_weight", flow_weight)):
        if not 0.0 <= v < float("inf"):
            raise ValueError("vespcn step: %s %r is not a non-negative finite number" % (name, v))
    out = []

    def weighted(weight, device):
        if ops._LOSS_SEED[0] is None and 0.0 < weight < 1.0:
            return ops.loss_seed(weight, ops._const_scalar(weight, device))
        return contextlib.nullcontext()

    def fwd_bwd(frames, target):
        opt.zero_grad()
        with _seeded(dp):
            with weighted(mc_weight, frames.device):      # (the only loss node inside the net is motion_fuse's)
                sr, mc, flow = model.forward_terms(frames)
            with weighted(flow_weight, frames.device):
                smooth = ops.flow_huber_loss(flow)
            loss = ops.loss_sum(ops.loss_sum(ops.mse_loss(sr, target), mc, 1.0, mc_weight), smooth, 1.0, flow_weight)
        _backward(loss, dp)
        out.append(loss)
        return loss

    def update(*batch):
        opt.step()
        return out.pop()

    return [(fwd_bwd, dp), (update, None)]


def vespcn_step(model, opt, mc_weight=0.01, flow_weight=0.001, dp=None):
    """The eager closure of `vespcn_segments` (see there); it carries `segments`, so the common capture takes it."""
    return eager_step(vespcn_segments(model, opt, mc_weight, flow_weight, dp))


def drcn_step(model, opt, w_opt, alpha_dev, beta, reg_dev=None):
    """drcn.py:196-221: zero_grad -> forward -> loss = alpha * mean_d MSE(y_d, t) + (1 - alpha) * MSE(out, t)
    + beta * sum_theta sum theta^2 (R of the parameters BEFORE the update; w excluded) -> backward -> Adam on the model's
    flat buffer and on w.  alpha_dev: the epoch's alpha as a 0-dim device tensor (the trainer rewrites it between epochs,
    a captured step reads the new value).  The reg term's gradient 2 * beta * theta is added to the flat gradient after
    the backward pass (one srk_axpby), so `.grad` is what the reference's loss.backward() leaves."""
    reg_dev = torch.zeros((), dtype=torch.float32, device=alpha_dev.device) if reg_dev is None else reg_dev

    def step(inp, target):
        opt.zero_grad()
        ops.sumsq(opt.flat.data, beta, out=reg_dev)
        loss = ops.drcn_head(model.reconstructions(inp), inp, model.w, target, alpha_dev, reg_dev)
        _backward(loss, None)
        ops.add_scaled_(opt.flat.grad, opt.flat.data, 2.0 * beta)
        opt.step()
        w_opt.step()
        return loss
    return step


def srgan_step(G, D, g_opt, d_opt, g_dp=None, d_dp=None, feature_extractor=None, lazy_pack=False, prune_dead_grads=False,
               perceptual=False, vgg_weight=6e-3):
    """srgan.py:249-310 with [B,1] labels, as the eager closure of `srgan_segments` (see there for the arguments)."""
    return eager_step(srgan_segments(G, D, g_opt, d_opt, g_dp, d_dp, lazy_pack, feature_extractor, prune_dead_grads,
                                     perceptual, vgg_weight))


def srgan_segments(G, D, g_opt, d_opt, g_dp=None, d_dp=None, lazy_pack=False, feature_extractor=None,
                   prune_dead_grads=False, perceptual=False, vgg_weight=6e-3):
    """The adversarial step, srgan.py:249-310 with [B,1] labels, cut at its two gradient exchanges:
    [(D forward/backward, d_dp), (D update + G forward/backward, g_dp), (G update, None)] -> (d_loss, g_loss).
    As in the reference the D step back-propagates through G (G is not detached, srgan.py:279) and the G step accumulates
    into D's gradients, which the next D step's zero_grad discards.
    `feature_extractor` (models.FeatureExtractor): adds the reference's VGG content term 6e-3 * MSE(vgg(norm(recon.data)),
    vgg(norm(hr)).detach()) to the reported G loss (srgan.py:301-308).  Both operands are detached in the reference,
    so the term changes the logged scalar only — never a gradient; without an extractor the step
    returns mse + 1e-3 * GAN, which has the same gradients.  `vgg_weight` replaces the 6e-3.
    perceptual (NOT the reference's execution, off by default): the term stays attached to G's output,
    g_loss = mse + 1e-3 * GAN + vgg_weight * ops.perceptual_loss(recon, hr, feature_extractor), and trains the generator
    -- the loss the SRGAN paper is about.  It needs an extractor.  The extractor's parameters are frozen (data gradients
    only; nothing joins a flat buffer or an exchange); the three gradients of recon are added by srk_axpby (ops.fork).
    As in the logged term the batch arrives normalised and the term normalises it again (srgan.py:193-194,302-303).
    lazy_pack: the two zero_grad() calls skip the filter pack of a model whose plan is current (optim.zero_grad,
    repack="stale": 2 instead of 4 whole-model packs per step) -- for steps replayed by a graph that knows both
    FlatParams (GraphedFn(flats=[...]) / GraphedSegments).
    prune_dead_grads (NOT the reference's execution, off by default and in bench.py's c5): the reference computes two sets
    of gradients nobody reads -- G's from D_loss.backward() (G_optimizer.zero_grad() clears them before the G step,
    srgan.py:287-291) and D's parameter gradients from G_loss.backward() (cleared by the next iteration's
    D_optimizer.zero_grad(), srgan.py:272).  With the flag the D step sees G's output detached and the G step runs D
    with its parameters frozen (data gradients only).  Parameters, optimizer states and BatchNorm statistics after the
    step are the faithful step's (up to the summation order inside the grouped weight-gradient launches, whose split
    depends on how many layers share a launch); D's `.grad` then holds the D step's gradients only.  The flag is
    honoured by every form of the step, the split-graph data-parallel one included."""
    from . import utils
    vgg_weight = float(vgg_weight)
    if perceptual and feature_extractor is None:
        raise ValueError("srgan step: perceptual=True needs a feature_extractor (models.FeatureExtractor)")
    if not vgg_weight >= 0.0:
        raise ValueError("srgan step: vgg_weight %r is negative" % (vgg_weight,))
    out = {}
    repack = "stale" if lazy_pack else "always"
    d_params = [p for p in D.parameters()] if prune_dead_grads else []

    def freeze_d(flag):
        for p in d_params:
            p.requires_grad_(not flag)

    def seg_d(lr_img, hr_img):
        b = lr_img.shape[0]
        real = ops.const_rows(1.0, b, lr_img.device)     # persistent label rows and srk_axpby loss sums: the captured
        fake = ops.const_rows(0.0, b, lr_img.device)     # step holds no ATen arithmetic node
        d_opt.zero_grad(repack=repack)
        recon_d = G(lr_img)      # (in grad mode either way: the same kernels and precision class as the reference path)
        out["d"] = ops.loss_sum(ops.bce_loss(D(hr_img), real),
                                ops.bce_loss(D(recon_d.detach() if prune_dead_grads else recon_d), fake))
        del recon_d              # (a local, not in `out`: it dies before the D backward ends)
        _backward(out["d"], d_dp)
        return out["d"]

    def seg_g(lr_img, hr_img):
        real = ops.const_rows(1.0, lr_img.shape[0], lr_img.device)
        d_opt.step()
        g_opt.zero_grad(repack=repack)
        recon = G(lr_img)
        if perceptual:   # three consumers: their gradients are added by srk_axpby, not by autograd's ATen add
            recon, rest = ops.fork(recon)
            rest, recon_vgg = ops.fork(rest)
        else:
            rest = recon
        freeze_d(True)
        try:
            gan_loss = ops.bce_loss(D(recon), real)
        finally:
            freeze_d(False)
        g_loss = ops.loss_sum(ops.mse_loss(rest, hr_img), gan_loss, 1.0, 1e-3)
        if perceptual:
            vgg_loss = ops.weighted_term(lambda p, t: ops.perceptual_loss(p, t, feature_extractor), vgg_weight,
                                         recon_vgg, hr_img)
            g_loss = ops.loss_sum(g_loss, vgg_loss, 1.0, vgg_weight)
        elif feature_extractor is not None:
            with torch.no_grad():   # srgan.py:301-305 (the inputs are already normalised once, as in the reference)
                real_feature = feature_extractor(utils.norm(hr_img, vgg=True))
                fake_feature = feature_extractor(utils.norm(recon.detach(), vgg=True))
                vgg_loss = ops.mse_loss(fake_feature, real_feature)
            g_loss = ops.loss_sum(g_loss, vgg_loss, 1.0, vgg_weight)
        _backward(g_loss, g_dp)
        out["g"] = g_loss
        return g_loss

    def seg_u(lr_img, hr_img):
        g_opt.step()
        return out.pop("d"), out.pop("g")

    return [(seg_d, d_dp), (seg_g, g_dp), (seg_u, None)]


def esrgan_step(G, D, g_opt, d_opt, feature_extractor, pixel_weight=1e-2, vgg_weight=1.0, gan_weight=5e-3,
                gan_type='ragan', vgg_layers=None):
    """The adversarial step of ESRGAN as the eager closure of `esrgan_segments` (see there)."""
    return eager_step(esrgan_segments(G, D, g_opt, d_opt, feature_extractor, pixel_weight, vgg_weight, gan_weight,
                                      gan_type, vgg_layers))


GAN_TYPES = ("ragan", "vanilla")


def esrgan_segments(G, D, g_opt, d_opt, feature_extractor, pixel_weight=1e-2, vgg_weight=1.0, gan_weight=5e-3,
                    gan_type='ragan', vgg_layers=None):
    """ESRGAN's adversarial step (Wang et al., ECCV-W 2018) in the order BasicSR's model runs it, for batches in [0, 1]:
      G step, D's parameters frozen:   fake = G(lr)
          g_loss = pixel_weight * L1(fake, hr) + vgg_weight * L1(vgg(norm(fake)), vgg(norm(hr)))
                   + gan_weight * ragan(D(hr).detach(), D(fake), for the generator)          backward, g_opt.step()
      D step:   d_loss = ragan(D(hr), D(fake.detach()), for the discriminator)              backward, d_opt.step()
    -> (d_loss, g_loss), the order srgan_segments returns them in.  ragan = ops.ragan_loss, the relativistic average loss on
    D's logits (models.ESRGANDiscriminator) with the gradient through both batch means -- the paper's and the original
    code's D step, not BasicSR's later split one.  feature_extractor: models.FeatureExtractor(feature_layer=34), conv5_4
    before its ReLU; its term is ops.perceptual_loss(criterion='l1') and normalises the batch once.  D runs in training
    mode throughout (its BatchNorm statistics move in both steps, as there).  The three gradients of `fake` are added by
    srk_axpby (ops.fork) and the loss terms by ops.loss_sum with each weight folded into its loss kernel
    (ops.weighted_term): no ATen arithmetic node in a captured step.  One GPU: two segments without an exchange.
    gan_type 'vanilla' (BasicSR's SRGAN order, what Real-ESRGAN trains models.UNetDiscriminatorSN with): the term is
    ops.gan_logit_loss on D's logits of any shape,
      G step, D frozen:   gan_weight * gan(D(fake), real)            (D(hr) is not evaluated)
      D step:             d_loss = gan(D(hr), real) + gan(D(fake.detach()), fake), the sum and not the half.
    A U-Net discriminator's logit map is refused with 'ragan' (gan_type: the relativistic loss takes one logit a sample).
    vgg_layers (None: the single conv5_4 term above): an ordered mapping {'conv1_2': 0.1, ...}; the feature term is then
    Real-ESRGAN's, vgg_weight * ops.vgg_feature_loss(fake, hr, feature_extractor, vgg_layers), and the extractor must reach
    the deepest named layer."""
    from . import models
    if gan_type not in GAN_TYPES:
        raise ValueError("esrgan step: gan_type %r is not one of %s" % (gan_type, ", ".join(GAN_TYPES)))
    if gan_type == "ragan" and isinstance(D, models.UNetDiscriminatorSN):
        raise ValueError("esrgan step: gan_type 'ragan' with a U-Net discriminator: the relativistic average loss takes one "
                         "logit a sample, not a logit map (use gan_type='vanilla', main.py --gan_type vanilla)")
    vanilla = gan_type == "vanilla"
    pixel_weight, vgg_weight, gan_weight = float(pixel_weight), float(vgg_weight), float(gan_weight)
    if feature_extractor is None:
        raise ValueError("esrgan step: needs a feature_extractor (models.FeatureExtractor(feature_layer=34) with its weights)")
    for name, v in (("pixel_weight", pixel_weight), ("vgg_weight", vgg_weight), ("gan_weight", gan_weight)):
        if not 0.0 <= v < float("inf"):
            raise ValueError("esrgan step: %s %r is not a non-negative finite number" % (name, v))
    out = {}
    d_params = [p for p in D.parameters()]

    def freeze_d(flag):
        for p in d_params:
            p.requires_grad_(not flag)

    if vgg_layers is not None:
        vgg_layers = dict((name, w) for name, _, w in ops.vgg_layer_plan(vgg_layers, feature_extractor.VGG19_CFG))

    def percep(pred, target):
        if vgg_layers is not None:
            return ops.vgg_feature_loss(pred, target, feature_extractor, vgg_layers, normalize=True)
        return ops.perceptual_loss(pred, target, feature_extractor, normalize=True, criterion='l1')

    def gan_g(fake_logits, real_logits):
        return ops.ragan_loss(real_logits, fake_logits, True)

    def seg_g(lr_img, hr_img):
        g_opt.zero_grad()
        fake = G(lr_img)
        f_gan, rest = ops.fork(fake)       # three consumers: their gradients are added by srk_axpby
        f_pix, f_vgg = ops.fork(rest)
        out["fake"] = fake.detach()
        freeze_d(True)
        try:
            if vanilla:
                l_gan = ops.weighted_term(lambda p, t: ops.gan_logit_loss(p, True), gan_weight, D(f_gan), None)
            else:
                real_logits = D(hr_img).detach()
                l_gan = ops.weighted_term(gan_g, gan_weight, D(f_gan), real_logits)
        finally:
            freeze_d(False)
        l_pix = ops.weighted_term(ops.l1_loss, pixel_weight, f_pix, hr_img)
        l_vgg = ops.weighted_term(percep, vgg_weight, f_vgg, hr_img)
        g_loss = ops.loss_sum(ops.loss_sum(l_pix, l_vgg, pixel_weight, vgg_weight), l_gan, 1.0, gan_weight)
        _backward(g_loss, None)
        g_opt.step()
        out["g"] = g_loss
        return g_loss

    def seg_d(lr_img, hr_img):
        d_opt.zero_grad()
        if vanilla:
            d_loss = ops.loss_sum(ops.gan_logit_loss(D(hr_img), True), ops.gan_logit_loss(D(out.pop("fake")), False))
        else:
            d_loss = ops.ragan_loss(D(hr_img), D(out.pop("fake")), False)
        _backward(d_loss, None)
        d_opt.step()
        return d_loss, out.pop("g")

    return [(seg_g, None), (seg_d, None)]


def _capture(graph, pool=None):
    """torch.cuda.graph with capture_error_mode="thread_local": ProcessGroupNCCL's watchdog thread polls the events of
    earlier collectives (hipEventQuery) at its own pace, and under the default "global" mode a query that lands while
    THIS thread is capturing is an illegal call that takes the process down -- seen on MI355X as an intermittent abort
    of the first capture after a broadcast / all-reduce (tests/test_dp_gpu.py, single-rank RCCL).  Work the autograd
    thread launches on the capturing stream is captured in either mode."""
    ops.amax_new_step()   # running maxima computed before the capture must not be baked into it
    return torch.cuda.graph(graph, pool=pool, capture_error_mode="thread_local")


class _Splitter(object):
    """Captures a function as a SEQUENCE of hipGraphs cut at the collectives it issues through ops._collective (SyncBN:
    one all-reduce of the [2C] sums per BatchNorm call and direction): items = [("graph", g) | ("eager", fn), ...].
    The backward pass runs on the calling thread while capturing (torch.autograd.set_multithreading_enabled(False)):
    a capture has to be ended by the thread that began it."""

    def __init__(self, pool):
        self.pool, self.items, self.g = pool, [], None

    def begin(self):
        self.g = torch.cuda.CUDAGraph()
        self.g.capture_begin(pool=self.pool, capture_error_mode="thread_local")

    def end(self):
        self.g.capture_end()
        self.pool = self.g.pool()
        self.items.append(("graph", self.g))
        self.g = None

    def collective(self, fn):
        self.end()
        fn()                       # (keeps the process group's sequence numbers in step with the other ranks)
        self.items.append(("eager", fn))
        self.begin()

    def capture(self, fn, args):
        ops.amax_new_step()
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        ops._SPLITTER[0] = self
        try:
            with torch.cuda.stream(side), torch.autograd.set_multithreading_enabled(False):
                self.begin()
                try:
                    out = fn(*args)
                finally:
                    self.end()
        finally:
            ops._SPLITTER[0] = None
        cur.wait_stream(side)
        return out


def _has_sync_bn(segments):
    for _, dp in segments:
        mod = getattr(getattr(dp, "flat", None), "module", None)
        if mod is not None and any(getattr(m, "sync_group", None) is not None for m in mod.modules()):
            return True
    return False


def sync_batchnorm(module, group=None):
    """SyncBN (SURVEY.md 8e caveat): every BatchNorm of `module` all-reduces its [2C] sums over `group` (None: the default
    process group), so a data-parallel step normalises with the statistics of the GLOBAL batch, like the single-process
    reference; no-op without an initialised process group.  Returns the number of layers switched."""
    import torch.distributed as dist
    from .layers import BatchNorm1d, BatchNorm2d
    if not dist.is_initialized():
        return 0
    grp = group if group is not None else dist.group.WORLD
    n = 0
    for m in module.modules():
        if isinstance(m, (BatchNorm2d, BatchNorm1d)):
            m.sync_group = grp
            n += 1
    return n


class GraphedSegments(object):
    """A train step as hipGraphs with static input buffers: THE capture of this package.

    `segments` = [(fn(*inputs), dp or None), ...] (see the module docstring): `warmup` eager steps on a side stream,
    then every fn is captured as one graph (cut again at every statistics all-reduce under SyncBN: _Splitter).  A
    segment with an active DataParallel ends in a backward pass whose weight gradients were left pending
    (ops.manual_wgrad_flush): each pending launch group becomes a small graph of its own, and at replay the groups run
    one after the other with the RCCL all-reduce of the bucket each one completes issued (eagerly, async) right behind
    it — the bucket travels while the next group computes.  `flats`: the FlatParams the step updates, beside those of
    its dps — their PackPlans and the packed-filter caches of no-grad forwards (layers._PackCache) are invalidated after
    every replay, which changed the weights without optim.step()'s host bookkeeping, and what somebody else changed
    between two replays is re-packed in front of the next (_repack_touched).  Call with new batches (copied into the
    static buffers, `.static`); returns what the last fn returned."""

    def __init__(self, segments, example_inputs, warmup=2, flats=()):
        self.static = _static_buffers(example_inputs)
        self.segments = segments
        eager = eager_step(segments)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                eager(*self.static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.plan, pool = [], None
        split = _has_sync_bn(segments)    # SyncBN: the segment's graph is cut again at every statistics all-reduce
        with _no_gc_during_capture():
            for fn, dp in segments:
                if split:
                    sp = _Splitter(pool)
                    self.out = sp.capture(fn, self.static)
                    pool, g = sp.pool, sp.items
                else:
                    g = torch.cuda.CUDAGraph()
                    with _capture(g, pool=pool):
                        self.out = fn(*self.static)
                    pool = g.pool()
                    g = [("graph", g)]
                wgraphs, sends, keep = [], [], None
                if _active(dp):
                    keep = ops.pending_wgrad_groups(dp.trunk_chunk_layers)   # holds x / dy / mask tensors of graph `g` alive
                    sends = dp.plan(keep)
                    ops.drop_pending_wgrads()
                    for recs in keep:
                        wg = torch.cuda.CUDAGraph()
                        with _capture(wg, pool=pool):
                            ops.launch_wgrad_group(recs)
                        wgraphs.append(wg)
                else:
                    ops.flush_wgrads()
                self.plan.append((g, dp, wgraphs, sends, keep))
        self._flats = []
        for f in list(flats) + [dp.flat for _, dp in segments if dp is not None]:
            if hasattr(f, "mark_changed") and not any(f is g for g in self._flats):
                self._flats.append(f)
        self._seen = {}
        self._after_replay()   # same host bookkeeping as after a replay

    def close(self):
        """Drop the captured graphs now (outside any capture) instead of whenever the garbage collector finds them."""
        self.plan = []

    def _after_replay(self):
        bump_weight_epoch()
        for f in self._flats:
            f.mark_changed()
        _note_epochs(self._flats, self._seen)

    def __call__(self, *batch):
        for s, b in zip(self.static, batch):
            if b is not s:
                s.copy_(b, non_blocking=True)
        _repack_touched(self._flats, self._seen)
        for items, dp, wgraphs, sends, _ in self.plan:
            for kind, obj in items:
                if kind == "graph":
                    obj.replay()
                else:
                    obj()
            if _active(dp):
                works = []
                if not wgraphs:
                    dp.send(sends[0] if sends else [(0, dp.flat.grad.numel())], works)
                for wg, ranges in zip(wgraphs, sends):
                    wg.replay()
                    dp.send(ranges, works)
                for w in works:
                    w.wait()
        self._after_replay()
        return self.out


def _graph_segments(step):
    """The segments an eager step is captured as: its own where one of them has an exchange to be cut at, else the whole
    step as ONE graph (a single-GPU step stays one graph launch; a closure without segments cannot be split)."""
    segments = getattr(step, "segments", None)
    if segments and any(_active(dp) for _, dp in segments):
        return segments
    return [(step, None)]


def capture_step(step, example_inputs, warmup=3, flats=()):
    """The hipGraph form of an eager step (any closure of this module, or any function of tensors that is stream work
    only): split at the gradient exchanges where it has segments with an active DataParallel, else one graph."""
    return GraphedSegments(_graph_segments(step), example_inputs, warmup, flats)


class GraphedFn(GraphedSegments):
    """hipGraph capture of an arbitrary single-GPU step function of tensors (e.g. the two-model, two-optimizer SRGAN
    step, `srgan_step` without data parallelism) as ONE graph.  Everything the step does must be stream work (no host
    reads of device values), which holds for all steps of this package."""

    def __init__(self, fn, example_inputs, warmup=3, flats=()):
        super(GraphedFn, self).__init__([(fn, None)], example_inputs, warmup, flats)


class GraphedStep(GraphedSegments):
    """hipGraph capture of the loss step (`loss_segments`).

    Single GPU: one graph = zero_grad + filter packing + forward + loss + backward (data-gradient chain, then the
    grouped weight gradients) + [clip] + optimizer.  Data parallel: graph A (through the data-gradient chain), one small
    graph per weight-gradient group with its gradient bucket's RCCL all-reduce issued behind it, then graph B = [clip] +
    optimizer."""

    def __init__(self, model, opt, loss_fn, example_inputs, dp=None, clip=None, warmup=3):
        step = eager_step(loss_segments(model, opt, loss_fn, dp, clip))
        super(GraphedStep, self).__init__(_graph_segments(step), example_inputs, warmup, [opt.flat])

    seg = property(lambda self: self)   # (the split capture used to be a member of this name: `step.seg.plan` still reads)


# The kinds that train on a loss of their own (SRGAN and ESRGAN on adversarial content terms, DRCN through its fused
# recursive-supervision head): mixed_loss's terms are refused for them, here and by sr_trainers' flag checks.
OWN_LOSS_KINDS = ("srgan", "drcn", "esrgan")
VESPCN_TERMS = {"mc_weight": 0.01, "flow_weight": 0.001}   # the paper's values as remembered, unchecked


def build(kind, model, lr, dp_group=None, use_dp=False, ema_decay=0.0, **terms):
    """(flat, optimizer, dp, step) for one of 'srcnn' | 'fsrcnn' | 'vdsr' | 'edsr' | 'lapsrn' | 'espcn' | 'rcan' | 'rdn' | 'swinir': the one place that
    names the loss and the clip a kind trains with.  terms: mixed_loss's keywords (ssim_weight, fft_weight, fft_norm,
    lpips_weight, lpips_net; RGB models only, refused for OWN_LOSS_KINDS), each of which at 0 leaves the step as it is
    without the argument.  ema_decay d in (0, 1): the optimizer keeps the moving average of the weights (`opt.ema`); it is
    updated inside opt.step()'s kernel, so eager steps, segments and graphs all carry it without a node of its own, and
    under data parallelism every rank's shadow is the same (same parameters, same kernel)."""
    from .dp import DataParallel
    if float(terms.get("lpips_weight", 0.0)) > 0.0 and kind in OWN_LOSS_KINDS:
        raise ValueError("lpips_weight %r: %s trains on a loss of its own and has no LPIPS term" % (terms["lpips_weight"], kind))
    flat = FlatParams(model)
    opt = make_optimizer(kind, flat, lr, ema_decay=ema_decay)
    dp = DataParallel(flat, dp_group) if use_dp else None
    if dp is not None:
        dp.broadcast_params()
        opt.ema_reset()      # (the shadow starts as a copy of the parameters every rank now has)
    if kind == "vespcn":   # ESPCN's optimizer rule (optim.make_optimizer); its own three-term loss
        own = {k: terms.pop(k, v) for k, v in VESPCN_TERMS.items()}
        extra = sorted(k for k, v in terms.items() if k in ("ssim_weight", "fft_weight", "lpips_weight") and v)
        if extra:
            raise ValueError("%s: vespcn trains on MSE + mc + flow smoothness and has no such term" % ", ".join(extra))
        return flat, opt, dp, vespcn_step(model, opt, dp=dp, **own)
    if kind in ("edsr", "rcan", "rdn", "swinir"):
        return flat, opt, dp, l1_step(model, opt, dp, **terms)
    if kind == "lapsrn":
        return flat, opt, dp, lapsrn_step(model, opt, dp, **terms)
    return flat, opt, dp, mse_step(model, opt, dp, clip=0.4 if kind == "vdsr" else None, **terms)


def _repack_touched(flats, seen):
    """Before a replay: a captured multi-model step packs a model's filters only where ITS OWN updates made them stale
    (optim.zero_grad skips a current plan), so parameters somebody else changed since the last replay -- anything that
    went through FlatParams.mark_changed(): load_state_dict (post-hook registered by FlatParams), DataParallel's
    broadcast, an eager optimizer step in between; a raw write to `.data` needs an explicit mark_changed() -- are
    re-packed here, eagerly, in front of the graph."""
    for f in flats:
        if seen.get(id(f)) != f.epoch and not f.plan.current():
            f.plan.pack()


def _note_epochs(flats, seen):
    for f in flats:
        seen[id(f)] = f.epoch


class AutoGraph(object):
    """A train step that turns itself into a hipGraph.  The FIRST batch of a shape runs through `eager` (a real step, and
    every lazy initialisation happens outside a capture); the next batch of that shape is captured by
    `make_graph(tensors)` (capture_step or one of the Graphed* classes, with warmup=0 on that batch) and replayed
    from then on.  Batches of another shape (the ragged last one of an epoch) run eagerly.  Learning rates are device
    scalars the optimizer kernels read (optim._Group: `group['lr'] /= 2` reaches them), so a decay needs no re-capture.
    `enabled=False`: always eager."""

    def __init__(self, eager, make_graph, enabled=True):
        self.eager, self.make_graph, self.enabled = eager, make_graph, enabled
        self.graph, self.seen = None, None

    def __call__(self, *tensors):
        if not self.enabled or not all(t.is_cuda for t in tensors):
            return self.eager(*tensors)
        shapes = tuple(tuple(t.shape) for t in tensors)
        g = self.graph
        if g is not None and g[1] == shapes:
            return g[0](*tensors)
        if self.seen != shapes:                 # first batch of this shape: eager (and remember the shape)
            if self.seen is None or g is None:
                self.seen = shapes
            return self.eager(*tensors)
        self.close()
        gs = self.make_graph(tensors)
        self.graph = (gs, shapes)
        return gs(*tensors)

    def close(self):
        if self.graph is not None and hasattr(self.graph[0], "close"):
            self.graph[0].close()
        self.graph = None

