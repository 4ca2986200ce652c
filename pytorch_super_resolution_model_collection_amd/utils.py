"""Tensor-side helpers of the reference's utils.py that sit on the training loop: weight
initialisers (utils.py:76-113), border crop (`shave`, :197-205), PSNR (:208-216), the
mean/std normalisation constants (:219-239), and save_img (:116-131).  Plotting / GIF helpers are out of scope
(SURVEY.md §2 rows 11-12)."""
import os

import torch


def _init_by_classname(m, conv_linear_init, norm_init):
    name = m.__class__.__name__
    if any(name.find(k) != -1 for k in ("Linear", "Conv2d", "ConvTranspose2d")):
        conv_linear_init(m.weight)
        if getattr(m, "bias", None) is not None:
            m.bias.data.zero_()
    elif name.find("Norm") != -1 and getattr(m, "weight", None) is not None:
        # (parameter-free norms — InstanceNorm2d's default — have nothing to initialise; the reference's
        #  `m.weight.data.normal_` would raise on them, utils.py:89)
        norm_init(m.weight)
        if m.bias is not None:
            m.bias.data.zero_()


def weights_init_normal(m, mean=0.0, std=0.02):
    """utils.py:76-93: N(mean, std) for Linear/Conv2d/ConvTranspose2d weights, zero bias,
    N(1, 0.02) for *Norm* weights — matched by class NAME exactly like the reference."""
    _init_by_classname(m, lambda w: w.data.normal_(mean, std), lambda w: w.data.normal_(1.0, 0.02))


def weights_init_kaming(m):
    """utils.py:96-113 (kaiming-normal, fan_in, gain sqrt(2))."""
    _init_by_classname(m, lambda w: torch.nn.init.kaiming_normal_(w), lambda w: w.data.normal_(1.0, 0.02))


def shave(imgs, border_size=0):
    """utils.py:197-205: crop `border_size` pixels from every side (a view; no copy needed)."""
    if border_size == 0:
        return imgs
    return imgs[..., border_size:-border_size, border_size:-border_size]


def PSNR(pred, gt):
    """utils.py:208-216 (prediction clamped to [0,1], peak 1.0; 100 for identical images).  GPU tensors: computed on
    the device by srk_psnr and returned as a 0-dim DEVICE tensor — no host copy and no sync per image (float() it, or
    torch.stack a list of them, when the numbers are needed).  CPU tensors (what the reference passes) are moved to the
    current device first; there is no host arithmetic."""
    from . import ops
    if not pred.is_cuda:
        pred = pred.to("cuda")
    return ops.psnr(pred.float(), gt.to(pred.device).float())[0]


def SSIM(pred, gt, shave=0, domain='float'):
    """Structural similarity of pred against gt (ops.ssim: 11 x 11 Gaussian window, valid positions, mean over planes),
    computed on the device and returned as a 0-dim DEVICE tensor, like PSNR.  shave crops that many pixels from each
    side first; domain 'float' compares what PSNR compares, 'u8' the 8-bit picture save_img writes, 'y8' its luma."""
    from . import ops
    if not pred.is_cuda:
        pred = pred.to("cuda")
    return ops.ssim(pred.float(), gt.to(pred.device).float(), shave, domain)[0]


def load_niqe_params(path):
    """The pristine model of NIQE from an .npz file: (mu_p [36], cov_p [36, 36]) as float64 arrays.  Keys: `mu_pris_param`
    ([36] or [1, 36]) and `cov_pris_param` -- the names BasicSR's niqe_pris_params.npz uses as remembered, not checked
    against that file; a `gaussian_window` key is ignored (the window is the kernel's own).  A missing key is named."""
    import numpy as np
    with np.load(os.fspath(path), allow_pickle=False) as f:
        missing = [k for k in ('mu_pris_param', 'cov_pris_param') if k not in f.files]
        if missing:
            raise KeyError("%s: no key %s (a NIQE parameter file holds mu_pris_param and cov_pris_param; it has %s)"
                           % (path, ' and '.join(repr(k) for k in missing), sorted(f.files)))
        mu, cov = np.asarray(f['mu_pris_param'], dtype=np.float64), np.asarray(f['cov_pris_param'], dtype=np.float64)
    if mu.size != 36 or cov.shape != (36, 36):
        raise ValueError("%s: mu_pris_param %s and cov_pris_param %s are not [36] (or [1, 36]) and [36, 36]"
                         % (path, mu.shape, cov.shape))
    return mu.reshape(36), cov


def save_niqe_params(path, mu_p, cov_p):
    """Write (mu_p, cov_p) as the .npz load_niqe_params reads (mu_pris_param as [1, 36])."""
    import numpy as np
    np.savez(os.fspath(path), mu_pris_param=np.asarray(mu_p, dtype=np.float64).reshape(1, 36),
             cov_pris_param=np.asarray(cov_p, dtype=np.float64).reshape(36, 36))


def pool_niqe_rows(per_picture, sharp=0.75):
    """NIQE's own fit from (features [blocks, 36], sharpness [blocks]) pairs, one per pristine picture: per picture the
    rows whose sharpness exceeds `sharp` times the picture's maximum and that hold no NaN are kept; returns (mu_p, cov_p,
    rows used) with mu_p the mean and cov_p np.cov of the pooled rows.  Fewer than 37 pooled rows is an error (a 36 x 36
    covariance of fewer is singular by construction)."""
    import numpy as np
    rows = []
    for feats, sharpness in per_picture:
        f = feats.detach().cpu().numpy() if torch.is_tensor(feats) else np.asarray(feats)
        s = sharpness.detach().cpu().numpy() if torch.is_tensor(sharpness) else np.asarray(sharpness)
        rows.append(f[(s > float(sharp) * s.max()) & ~np.isnan(f).any(axis=1)])
    rows = np.concatenate(rows) if rows else np.empty((0, 36))
    if rows.shape[0] < 37:
        raise ValueError("fit_niqe_params: %d blocks pass the sharpness rule, the 36 x 36 covariance needs at least 37 "
                         "(more or larger pictures, or a smaller block)" % rows.shape[0])
    return rows.mean(axis=0), np.cov(rows, rowvar=False), int(rows.shape[0])


def fit_niqe_params(pictures, block=96, sharp=0.75, host=False):
    """Fit NIQE's pristine model from pictures ([C,H,W] float32 or uint8 tensors, C in {1, 3}; moved to the current
    device unless host=True, which runs the host twin instead): (mu_p, cov_p, rows used), see pool_niqe_rows.  A
    picture with fewer than two blocks is an error that names its size."""
    from . import ops
    per = []
    for img in pictures:
        if host:
            per.append(ops.niqe_features_host(img, 0, block, sharpness=True))
        else:
            img = torch.as_tensor(img)
            per.append(ops.niqe_features(img if img.is_cuda else img.to("cuda"), 0, block, sharpness=True))
    return pool_niqe_rows(per, sharp)


class NIQE(torch.nn.Module):
    """NIQE (ops.niqe; Mittal et al. 2013, no reference picture, lower is better) as a metric: forward(img) returns the
    score of one picture [C,H,W] (float32 in [0, 1], read as the 8-bit picture save_img writes, or uint8) as a Python
    float.  params: a path for load_niqe_params, or (mu_p, cov_p)."""

    def __init__(self, params, shave=0, block=96):
        super(NIQE, self).__init__()
        self.params = load_niqe_params(params) if isinstance(params, (str, os.PathLike)) else (params[0], params[1])
        self.shave, self.block = int(shave), int(block)

    def forward(self, img):
        from . import ops
        if not img.is_cuda:
            img = img.to("cuda")
        return ops.niqe(img, self.params, self.shave, self.block)


class SSIMLoss(torch.nn.Module):
    """1 - SSIM(pred, target) as a training loss (ops.ssim_loss: the prediction unclamped, float domain, loss and gradient
    from one kernel launch); [N,C,H,W] CUDA tensors with planes of at least 11 x 11."""

    def forward(self, pred, target):
        from . import ops
        return ops.ssim_loss(pred, target.to(pred.device))


class FFTLoss(torch.nn.Module):
    """The L1 on the 2-D Fourier spectrum of pred - target as a training loss (ops.fft_loss: BasicSR's FFTLoss on a dense
    fp64 DFT, loss and gradient from one call); norm "backward" or "ortho" as torch.fft.fft2 names them.  [N,C,H,W] CUDA
    tensors with planes of at most 256 x 256."""

    def __init__(self, norm="backward"):
        super(FFTLoss, self).__init__()
        if norm not in ("backward", "ortho"):
            raise ValueError("FFTLoss: norm %r is not 'backward' or 'ortho'" % (norm,))
        self.norm = norm

    def forward(self, pred, target):
        from . import ops
        return ops.fft_loss(pred, target.to(pred.device), self.norm)


class LPIPS(torch.nn.Module):
    """LPIPS (ops.lpips: Zhang et al. 2018, the VGG variant) as a metric: forward(pred, target) returns the per-sample
    values [N] on the device, without a graph.  [N,3,H,W] tensors with H, W >= 16, in [0, 1] when `normalize`, else in
    [-1, 1]; net: models.LPIPS (held as a sub-module, its parameters stay frozen)."""

    def __init__(self, net, normalize=True):
        super(LPIPS, self).__init__()
        self.net = net
        self.normalize = bool(normalize)

    def forward(self, pred, target):
        from . import ops
        with torch.no_grad():
            return ops.lpips(pred.detach(), target.to(pred.device), self.net, self.normalize, reduce=False)


class LPIPSLoss(torch.nn.Module):
    """LPIPS as a training loss (ops.lpips, reduce=True): the mean over the batch, a 0-dim device tensor with the contract
    of the other losses; the gradient reaches pred only.  Arguments as utils.LPIPS."""

    def __init__(self, net, normalize=True):
        super(LPIPSLoss, self).__init__()
        self.net = net
        self.normalize = bool(normalize)

    def forward(self, pred, target):
        from . import ops
        return ops.lpips(pred, target.to(pred.device), self.net, self.normalize, reduce=True)


class PerceptualLoss(torch.nn.Module):
    """The VGG feature loss as a training loss (ops.perceptual_loss): MSE of `extractor`'s features of pred and target,
    each normalised with the VGG constants first when `normalize`; the gradient reaches pred only.  [N,3,H,W] CUDA
    tensors; extractor: models.FeatureExtractor (held as a sub-module, its parameters stay frozen)."""

    def __init__(self, extractor, normalize=True):
        super(PerceptualLoss, self).__init__()
        self.extractor = extractor
        self.normalize = bool(normalize)

    def forward(self, pred, target):
        from . import ops
        return ops.perceptual_loss(pred, target.to(pred.device), self.extractor, self.normalize)


class VGGFeatureLoss(torch.nn.Module):
    """Real-ESRGAN's multi-layer VGG feature loss as a training loss (ops.vgg_feature_loss): sum_k w_k * L1 of the VGG19
    maps of layer k before its ReLU.  layer_weights: an ordered mapping {'conv1_2': 0.1, ...}, checked here;
    extractor: models.FeatureExtractor reaching the deepest named layer (held as a sub-module, its parameters stay
    frozen).  [N,3,H,W] CUDA tensors; the gradient reaches pred only."""

    def __init__(self, layer_weights, extractor, normalize=True):
        super(VGGFeatureLoss, self).__init__()
        from . import ops
        plan = ops.vgg_layer_plan(layer_weights, extractor.VGG19_CFG)
        self.layer_weights = dict((name, weight) for name, _, weight in plan)
        self.extractor = extractor
        self.normalize = bool(normalize)

    def forward(self, pred, target):
        from . import ops
        return ops.vgg_feature_loss(pred, target.to(pred.device), self.extractor, self.layer_weights, self.normalize)


def save_img_name(img_num, save_dir='', is_training=False):
    """utils.py:126-130: the file a result image goes to."""
    return save_dir + ('/SR_result_epoch_{:d}' if is_training else '/SR_result_{:d}').format(img_num) + '.png'


def save_img(img, img_num, save_dir='', is_training=False):
    """utils.py:116-131: write the [C,H,W] (or [1,C,H,W]) result image, C = 1 or 3, as an 8-bit PNG under the reference's
    file name, and return that name.  The image is quantised on the device (ops.to_u8_image: clamp(0, 1) * 255,
    truncated -- for three channels the bytes of the reference's `(img * 255).clamp(0, 255).astype(uint8)`), copied to
    the host once and encoded by Pillow (the reference's scipy.misc.imsave no longer exists).  One-channel images are
    quantised the same way; the reference hands imsave a float array there, which that function stretched to the
    image's own min..max.  A CPU tensor is moved to the current device first, as in PSNR."""
    from PIL import Image
    from . import ops
    if not img.is_cuda:
        img = img.to("cuda")
    arr = ops.to_u8_image(img.float()).cpu().numpy()
    os.makedirs(save_dir or '.', exist_ok=True)
    save_fn = save_img_name(img_num, save_dir, is_training)
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(save_fn)
    return save_fn


VGG_MEAN = (0.485, 0.456, 0.406)
VGG_STD = (0.229, 0.224, 0.225)
VGG_DENORM_MEAN = (-2.118, -2.036, -1.804)
VGG_DENORM_STD = (4.367, 4.464, 4.444)


def norm(img, vgg=False):
    """utils.py:219-229 applied per channel on a [C,H,W] or [B,C,H,W] tensor (the reference's 4-D use is broken on
    its own stack; this is the intended arithmetic).  One kernel (srk_channel_affine), bit-equal
    to torchvision's Normalize (sub_(mean).div_(std))."""
    from . import ops
    mean, std = (VGG_MEAN, VGG_STD) if vgg else ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    return ops.channel_affine(img, mean, std)


def denorm(img, vgg=False):
    """utils.py:232-239: vgg -> Normalize(mean=[-2.118,-2.036,-1.804], std=[4.367,4.464,4.444]); else
    ((img + 1) / 2).clamp(0, 1) — written as (img - (-1)) / 2, the same two IEEE operations."""
    from . import ops
    if vgg:
        return ops.channel_affine(img, VGG_DENORM_MEAN, VGG_DENORM_STD)
    return ops.channel_affine(img, (-1.0,) * 8, (2.0,) * 8, clamp01=True)


def img_interp(imgs, scale_factor, interpolation='bicubic'):
    """utils.py:242-269 — the per-image PIL round trip (ToPILImage -> resize -> ToTensor) as GPU kernels,
    bit-exact with it (ops.img_interp)."""
    from . import ops
    return ops.img_interp(imgs, scale_factor, interpolation)


def print_network(net):
    """utils.py:14-20"""
    num_params = sum(p.numel() for p in net.parameters())
    print(net)
    print('Total number of parameters: %d' % num_params)
