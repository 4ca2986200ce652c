"""The reference's image-folder input pipeline (dataset.py:22-149, data.py:33-65) re-designed for the MI355X:

  host   : file listing, PNG/JPEG decode (Pillow, in a thread pool — decode releases the GIL), nothing else;
  PCIe   : the decoded uint8 image goes through a pinned staging buffer and an asynchronous H2D copy on the loader's own
           HIP stream (1 byte per sample instead of the 4-byte floats the reference's DataLoader hands over);
  device : every transform of `TrainDatasetFromFolder.__getitem__` — random bicubic re-scale (Pillow's 8-bit two-pass
           resampler, bit-exact: csrc/resize_pil.hip), RandomCrop, 90-degree rotations, flips, the HR / LR bicubic
           resizes, ToTensor and the ToPILImage -> bicubic -> ToTensor round trip of the "bicubic" image — as a handful of
           kernels per patch plus three batched resizes per minibatch.

Same classes / functions / argument names as the reference (`TrainDatasetFromFolder`, `TestDatasetFromFolder`,
`get_training_set`, `get_test_set`), same `(lr_img, hr_img, bc_img)` items, and the SAME calls to Python's `random` in the
same order, so `random.seed(s); ds[i]` picks the patch the reference would (parity: oracle/dataset_pil.py, bit-exact).
Reference quirk kept: with random_scale the whole image is first resized to crop x crop — the
"random crop" is then a no-op.  `is_gray` (convert('YCbCr'), dataset.py:85-86) is done by Pillow on the host on the
augmented 8-bit patch (one small D2H/H2D per patch, gray mode only): its integer colour matrix is Pillow's own.
Not provided: the BSDS300 HTTP download of data.py:9-30 (no network code in this package).
Beyond the reference: `Degradation` -- with `degrade=` set, the LR image is no longer the clean bicubic
shrink of the HR patch but LR = (HR * k) shrunk + n: a random anisotropic Gaussian blur in front of the shrink and Gaussian
noise behind it, both HIP kernels on the loader stream (csrc/degrade.hip), and with `jpeg_quality` JPEG compression of the
result (csrc/jpeg.hip).  Without it nothing changes, draws included.  `Degradation2` is
Real-ESRGAN's second-order chain in its place -- blur, resize, Gaussian or Poisson noise and JPEG, twice, then a sinc filter,
every stage a kernel from 8 bits to 8 bits -- and `usm=True` sharpens the 8-bit patches first (csrc/usm.hip).
"""
import ctypes
import math
import os
import random
from concurrent.futures import ThreadPoolExecutor
from os import listdir
from os.path import join

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr
from .ops import jpeg_subsampling as jpeg_subsampling_code

BICUBIC = 3  # PIL.Image.BICUBIC / srk_interp


def is_image_file(filename):
    """dataset.py:9-10"""
    return any(filename.endswith(extension) for extension in [".png", ".jpg", ".jpeg", ".bmp"])


def load_img(filepath):
    """dataset.py:13-15 — host decode to an RGB uint8 array [H, W, 3]."""
    from PIL import Image
    return np.asarray(Image.open(filepath).convert('RGB'), dtype=np.uint8)


def calculate_valid_crop_size(crop_size, scale_factor):
    """dataset.py:18-19"""
    return crop_size - (crop_size % scale_factor)


class _Null(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL = _Null()


def _stream_ptr(stream):
    return ctypes.c_void_p(stream.cuda_stream)


class _Device(object):
    """Device-side transforms on 8-bit images (thin wrappers over the C ABI), all on one HIP stream."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the input pipeline's transforms run on the GPU (got device %s); there is no CPU fallback"
                               % (device,))
        self.lib = _lib.load()
        self.stream = torch.cuda.Stream(device=self.device)
        self._sp = _stream_ptr(self.stream)
        self._ws_bytes = {}
        self._slab_buf, self._slab_off, self._depth = None, 0, 0

    # Every helper below runs on the loader stream.  PatchLoader enters the stream ONCE per batch (`batch()`); a
    # torch.cuda.stream context per call costs ~10 us of host time, three times per patch.
    def _on_stream(self):
        return _NULL if self._depth else torch.cuda.stream(self.stream)

    def batch(self):
        """Context of one batch: the loader stream is current, workspaces come from the start of the slab again."""
        dev = self

        class _Ctx(object):
            def __enter__(self_):
                self_.cm = torch.cuda.stream(dev.stream)
                self_.cm.__enter__()
                dev._depth += 1
                dev._slab_off = 0

            def __exit__(self_, *a):
                dev._depth -= 1
                return self_.cm.__exit__(*a)

        return _Ctx()

    def _slab(self, nbytes):
        nbytes = (nbytes + 255) & ~255
        if self._slab_buf is None or self._slab_off + nbytes > self._slab_buf.numel():
            # (out of room in the middle of a batch: a fresh slab; the old one is released to the loader stream's pool,
            #  whose reuse is ordered behind the kernels still reading it)
            self._slab_buf = torch.empty(max(64 << 20, 4 * nbytes), dtype=torch.uint8, device=self.device)
            self._slab_off = 0
        v = self._slab_buf[self._slab_off:self._slab_off + nbytes]
        self._slab_off += nbytes
        if not self._depth:
            self._slab_off = 0   # outside a batch context every call may reuse the slab (stream order protects it)
        return v

    # Pinned staging buffers are a ring allocated once and reused (pinning a fresh buffer per image is a driver call
    # of several milliseconds that also serialises against the device: 163 patches/s with it, see tools/loader_bench.py)
    RING = 64

    def upload(self, hwc):
        """HWC uint8 numpy -> device uint8 tensor through pinned memory, async on the loader stream."""
        if not hasattr(self, "_ring"):
            self._ring, self._ring_ev, self._ring_k = [None] * self.RING, [None] * self.RING, 0
        i = self._ring_k
        self._ring_k = (i + 1) % self.RING
        n = int(hwc.size)
        if self._ring_ev[i] is not None:
            self._ring_ev[i].synchronize()   # the copy that last used this slot (RING uploads ago) is done
        if self._ring[i] is None or self._ring[i].numel() < n:
            self._ring[i] = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
        pinned = self._ring[i][:n].view(hwc.shape)
        np.copyto(pinned.numpy(), hwc)
        with self._on_stream():
            d = torch.empty(hwc.shape, dtype=torch.uint8, device=self.device)
            d.copy_(pinned, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._ring_ev[i] = ev
        return d

    def resize(self, x, strides, planes, h, w, oh, ow, out_float, filt=BICUBIC):
        """Image.resize((ow, oh), BICUBIC) of `planes` 8-bit planes addressed by element strides (plane, row, pixel); filt:
        another of Pillow's filters (BILINEAR, BOX: the second-order chain draws it)."""
        lib = self.lib
        with self._on_stream():
            y = torch.empty((planes, oh, ow), dtype=torch.float32 if out_float else torch.uint8, device=self.device)
            key = (planes, h, w, oh, ow) if filt == BICUBIC else (planes, h, w, oh, ow, filt)
            nbytes = self._ws_bytes.get(key)
            if nbytes is None:
                nbytes = self._ws_bytes[key] = max(int(lib.srk_img_resize_u8_workspace_bytes(planes, h, w, oh, ow, filt)), 256)
            # one workspace per call (the calls of a batch are in flight together on the loader stream), drawn from a
            # slab that is re-used batch after batch
            ws = self._slab(nbytes)
            check(lib.srk_img_resize_u8(ptr(x), strides[0], strides[1], strides[2], ptr(y), int(out_float), planes, h, w,
                                        oh, ow, filt, ptr(ws), nbytes, self._sp), "srk_img_resize_u8")
        return y

    def augment(self, x, strides, c, h, w, crop, rot, fliplr, fliptb, out=None):
        """crop (x0, y0, cw, ch) -> rot x 90 deg ccw -> flips; planar uint8 [c, oh, ow]."""
        x0, y0, cw, ch = crop
        oh, ow = (cw, ch) if rot & 1 else (ch, cw)
        with self._on_stream():
            y = out if out is not None else torch.empty((c, oh, ow), dtype=torch.uint8, device=self.device)
            check(self.lib.srk_patch_augment_u8(ptr(x), strides[0], strides[1], strides[2], ptr(y), c, h, w, x0, y0, cw, ch,
                                                rot, int(fliplr), int(fliptb), self._sp), "srk_patch_augment_u8")
        return y

    def patch(self, img, c, h, w, scale, crop, rot, fliplr, fliptb, out=None):
        """Decoded interleaved image on the device -> augmented planar 8-bit patch (srk_patch_from_image_u8)."""
        x0, y0, cw, ch = crop
        oh, ow = (cw, ch) if rot & 1 else (ch, cw)
        sh, sw = (scale[1], scale[0]) if scale is not None else (0, 0)
        lib = self.lib
        with self._on_stream():
            y = out if out is not None else torch.empty((c, oh, ow), dtype=torch.uint8, device=self.device)
            key = ("patch", c, h, w, sh, sw)
            nbytes = self._ws_bytes.get(key)
            if nbytes is None:
                nbytes = self._ws_bytes[key] = int(lib.srk_patch_from_image_u8_workspace_bytes(c, h, w, sh, sw))
            ws = self._slab(nbytes)
            check(lib.srk_patch_from_image_u8(ptr(img), c, h, w, sh, sw, x0, y0, cw, ch, rot, int(fliplr), int(fliptb),
                                              ptr(y), ptr(ws), nbytes, self._sp), "srk_patch_from_image_u8")
        return y

    def bicubic_of_lr(self, lr, oh, ow):
        """ToPILImage -> Scale -> ToTensor on the float LR batch (dataset.py:98-99) = utils.img_interp's kernel."""
        lib = self.lib
        n, c, h, w = lr.shape
        with self._on_stream():
            y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=self.device)
            nbytes = int(lib.srk_img_interp_workspace_bytes(n, c, h, w, oh, ow, BICUBIC))
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            check(lib.srk_img_interp(ptr(lr), ptr(y), n, c, h, w, oh, ow, BICUBIC, ptr(ws), ws.numel(),
                                     self._sp), "srk_img_interp")
        return y

    def upload_f64(self, values):
        """Host fp64 numpy array -> device fp64 tensor, through the pinned ring like an image."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        return self.upload(values.reshape(-1).view(np.uint8)).view(torch.float64).view(values.shape)

    def blur(self, x, weights, planes_per_patch, b, h, w):
        """srk_blur_u8: dense 8-bit [b, planes_per_patch, h, w] under the fp64 tables weights [b, K, K] (device)."""
        with self._on_stream():
            y = torch.empty((b, planes_per_patch, h, w), dtype=torch.uint8, device=self.device)
            check(self.lib.srk_blur_u8(ptr(x), ptr(y), ptr(weights), planes_per_patch, b, h, w, int(weights.shape[-1]),
                                       self._sp), "srk_blur_u8")
        return y

    def noise(self, x, sigma, seed, b):
        """srk_noise_u8: dense 8-bit [b, ...] -> fp32 (x + sigma[b] * z) / 255 of the same shape; sigma fp64 [b] (device)."""
        with self._on_stream():
            y = torch.empty(x.shape, dtype=torch.float32, device=self.device)
            check(self.lib.srk_noise_u8(ptr(x), ptr(y), ptr(sigma), int(seed), b, x.numel() // b, self._sp), "srk_noise_u8")
        return y

    def noise_bytes(self, x, sigma, seed, b):
        """srk_noise_u8_bytes: noise() with the 8-bit level itself as the result, for the JPEG stage to follow."""
        with self._on_stream():
            y = torch.empty(x.shape, dtype=torch.uint8, device=self.device)
            check(self.lib.srk_noise_u8_bytes(ptr(x), ptr(y), ptr(sigma), int(seed), b, x.numel() // b, self._sp),
                  "srk_noise_u8_bytes")
        return y

    def jpeg(self, x, quality, subsampling, color, out_float=True):
        """srk_jpeg_u8: dense 8-bit [b, c, h, w] -> fp32 bytes / 255 of each patch compressed at quality[b] (fp64 on the
        device, 0 = left as it is) and decoded again; out_float False: the bytes themselves, for a stage to follow."""
        b, c, h, w = (int(v) for v in x.shape)
        with self._on_stream():
            y = torch.empty(x.shape, dtype=torch.float32 if out_float else torch.uint8, device=self.device)
            check(self.lib.srk_jpeg_u8(ptr(x), ptr(y), ptr(quality), c, b, h, w, int(subsampling), int(bool(color)),
                                       int(bool(out_float)), self._sp), "srk_jpeg_u8")
        return y

    def noise2(self, x, mode, gray, amount, cdf, seed, stage, color):
        """srk_noise2_u8: dense 8-bit [b, c, h, w] -> 8 bits under the per-patch fp64 mode, gray and amount [b] and the
        Poisson table cdf [256, 448], all on the device."""
        b, c, h, w = (int(v) for v in x.shape)
        with self._on_stream():
            y = torch.empty(x.shape, dtype=torch.uint8, device=self.device)
            check(self.lib.srk_noise2_u8(ptr(x), ptr(y), ptr(mode), ptr(gray), ptr(amount), ptr(cdf), int(seed), int(stage),
                                         b, c, h, w, int(bool(color)), self._sp), "srk_noise2_u8")
        return y

    def usm(self, x, g, weight, threshold):
        """srk_usm_u8: dense 8-bit [b, c, h, w] -> the unsharp-masked 8 bits; g fp64 [K] on the device."""
        b, c, h, w = (int(v) for v in x.shape)
        with self._on_stream():
            y = torch.empty(x.shape, dtype=torch.uint8, device=self.device)
            key = ("usm", b, c, h, w)
            nbytes = self._ws_bytes.get(key)
            if nbytes is None:
                nbytes = self._ws_bytes[key] = max(int(self.lib.srk_usm_u8_workspace_bytes(b, c, h, w)), 256)
            ws = self._slab(nbytes)
            check(self.lib.srk_usm_u8(ptr(x), ptr(y), ptr(g), int(g.numel()), float(weight), float(threshold), b, c, h, w,
                                      ptr(ws), nbytes, self._sp), "srk_usm_u8")
        return y

    def resident_f64(self, key, make):
        """A host-made fp64 table that goes up once and stays on the device (the Poisson table, the USM Gaussian)."""
        if not hasattr(self, "_tables"):
            self._tables = {}
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = self.upload_f64(make())
        return t

    def hand_over(self, *tensors):
        """Make the consumer's current stream wait for the loader stream; tensors become usable there."""
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self.stream)
        for t in tensors:
            t.record_stream(cur)
        return tensors


_HWC = lambda h, w, c: (1, w * c, c)       # element strides (plane, row, pixel) of an interleaved image
_CHW = lambda h, w: (h * w, w, 1)


BLUR_MAX_K = 21   # kBlurMaxK (csrc/degrade_common.h)


def blur_kernel_size(s1, s2):
    """Taps of the table of a blur with standard deviations s1, s2: 3 sigma to each side, capped at BLUR_MAX_K."""
    return min(BLUR_MAX_K, 2 * int(math.ceil(3 * max(s1, s2))) + 1)


def blur_weights(s1, s2, theta, K=None):
    """srk_blur_weights_host: the normalised K x K anisotropic Gaussian table (fp64 numpy); needs no GPU."""
    K = blur_kernel_size(s1, s2) if K is None else int(K)
    buf = (ctypes.c_double * (K * K))()      # (a ctypes array: numpy's .ctypes.data_as costs as much as the table itself)
    check(_lib.load().srk_blur_weights_host(float(s1), float(s2), float(theta), K, buf), "srk_blur_weights_host")
    w = np.frombuffer(buf, np.float64).reshape(K, K)
    return w


def _centred(tables, K):
    """The square tables (None = not blurred: the delta) centred among zeros in [B, K, K]."""
    out = np.zeros((len(tables), K, K), np.float64)
    for b, w in enumerate(tables):
        if w is None:
            out[b, K // 2, K // 2] = 1.0
        else:
            o = (K - w.shape[0]) // 2
            out[b, o:o + w.shape[0], o:o + w.shape[0]] = w
    return out


def _degrade_u8(dev, planes, weights, sigma, seed, oh, ow, quality=None, subsampling=1, color=True):
    """blur -> Pillow-exact bicubic shrink -> noise -> JPEG of dense 8-bit planes [B, C, H, W] on the loader stream.
    weights [B, K, K], sigma [B] and quality [B] (or None: no JPEG stage) are host fp64 arrays; they cross in one copy.  A
    batch without a blurred patch skips the blur (the delta table returns its input), one without noise takes the shrink's
    own bytes and one without a compressed patch (quality 0) the / 255 of the stage before: the same bits, fewer launches."""
    b, c, h, w = (int(v) for v in planes.shape)
    K = weights.shape[-1]
    blurred = bool((weights[:, K // 2, K // 2] != 1.0).any())
    noisy = bool((sigma != 0.0).any())
    jpeg = quality is not None and bool((quality != 0.0).any())
    if blurred or noisy or jpeg:
        params = dev.upload_f64(np.concatenate([weights.reshape(-1), sigma.reshape(-1)] + ([quality.reshape(-1)] if jpeg else [])))
    q = dev.blur(planes, params[:weights.size].view(b, K, K), c, b, h, w) if blurred else planes
    lr = dev.resize(q, _CHW(h, w), b * c, h, w, oh, ow, out_float=not (noisy or jpeg)).view(b, c, oh, ow)
    if noisy:
        lr = (dev.noise_bytes if jpeg else dev.noise)(lr, params[weights.size:weights.size + b], seed, b)
    return dev.jpeg(lr, params[weights.size + b:], subsampling, color) if jpeg else lr


def _check_jpeg_quality(q, what):
    if int(q) != q or not 1 <= int(q) <= 100:
        raise ValueError("%s must be a whole number in 1..100 (got %r)" % (what, q))
    return int(q)


class Degradation(object):
    """The classical degradation model of blind super-resolution, LR = (HR * k) shrunk + n: per patch,
    with probability `blur_prob`, an anisotropic Gaussian blur with standard deviations drawn from `blur_sigma` = (lo, hi)
    pixels and a uniform angle; then the loader's own bicubic shrink; then Gaussian noise of a standard deviation drawn
    from `noise_sigma` = (lo, hi) 8-bit levels (hi = 0: no noise, and no draw for it); then, with `jpeg_quality` = (lo, hi)
    set and with probability `jpeg_prob`, JPEG compression at a quality drawn from it and decoding again (DESIGN.md 24;
    `jpeg_subsampling` '4:2:0' as Pillow's default, or '4:4:4').  Draws come from Python's global `random`, after the
    batch's patch draws; those of the JPEG stage (draw_jpeg) after all others, and only when it is on."""

    def __init__(self, blur_prob=1.0, blur_sigma=(0.2, 4.0), noise_sigma=(0.0, 10.0), jpeg_quality=None, jpeg_prob=1.0,
                 jpeg_subsampling='4:2:0'):
        self.blur_prob = float(blur_prob)
        self.blur_sigma = (float(blur_sigma[0]), float(blur_sigma[1]))
        self.noise_sigma = (float(noise_sigma[0]), float(noise_sigma[1]))
        if not 0.0 <= self.blur_prob <= 1.0:
            raise ValueError("blur_prob must lie in [0, 1] (got %r)" % (blur_prob,))
        if not 0.0 < self.blur_sigma[0] <= self.blur_sigma[1] < float('inf'):
            raise ValueError("blur_sigma must be 0 < lo <= hi (got %r)" % (blur_sigma,))
        if not 0.0 <= self.noise_sigma[0] <= self.noise_sigma[1] < float('inf'):
            raise ValueError("noise_sigma must be 0 <= lo <= hi (got %r)" % (noise_sigma,))
        self.jpeg_quality, self.jpeg_prob = None, float(jpeg_prob)
        if jpeg_quality is not None:
            if len(jpeg_quality) != 2:
                raise ValueError("jpeg_quality must be (lo, hi) or None (got %r)" % (jpeg_quality,))
            self.jpeg_quality = tuple(_check_jpeg_quality(q, "jpeg_quality's bounds") for q in jpeg_quality)
            if self.jpeg_quality[0] > self.jpeg_quality[1]:
                raise ValueError("jpeg_quality must be lo <= hi (got %r)" % (jpeg_quality,))
        if not 0.0 <= self.jpeg_prob <= 1.0:
            raise ValueError("jpeg_prob must lie in [0, 1] (got %r)" % (jpeg_prob,))
        self.jpeg_subsampling = jpeg_subsampling_code(jpeg_subsampling)       # 1: 4:2:0, 0: 4:4:4

    def draw(self, batch):
        """(weights [B, K, K], sigma [B], seed) of one batch as host arrays.  Per patch: random() < blur_prob -> s1, s2,
        theta, else the delta; then sigma, only if noise is on; after the loop the 64-bit noise seed, only if noise is on.
        K is the batch's widest table (3 when no patch is blurred), narrower ones centred among zeros."""
        lo, hi = self.blur_sigma
        nlo, nhi = self.noise_sigma
        tables, sigma = [], np.zeros(batch, np.float64)
        for j in range(batch):
            if random.random() < self.blur_prob:
                s1, s2 = random.uniform(lo, hi), random.uniform(lo, hi)
                tables.append(blur_weights(s1, s2, random.uniform(0, math.pi)))
            else:
                tables.append(None)
            if nhi > 0:
                sigma[j] = random.uniform(nlo, nhi)
        seed = random.getrandbits(64) if nhi > 0 else 0
        K = max([w.shape[0] for w in tables if w is not None] + [3])
        return _centred(tables, K), sigma, seed

    def draw_jpeg(self, batch):
        """quality [B] of one batch as a host fp64 array (0: the patch is not compressed), or None when the JPEG stage is
        off -- then nothing is drawn.  Runs after draw().  Per patch: random() < jpeg_prob -> randint(lo, hi)."""
        if self.jpeg_quality is None:
            return None
        lo, hi = self.jpeg_quality
        quality = np.zeros(batch, np.float64)
        for j in range(batch):
            if random.random() < self.jpeg_prob:
                quality[j] = random.randint(lo, hi)
        return quality

    def apply(self, dev, patches, lr_sz, color=True):
        """Dense 8-bit patches [B, C, crop, crop] on the device -> the degraded fp32 lr [B, C, lr_sz, lr_sz].  color: the
        planes are R, G, B (else Y, Cb, Cr); only the JPEG stage asks."""
        weights, sigma, seed = self.draw(int(patches.shape[0]))
        quality = self.draw_jpeg(int(patches.shape[0]))
        if quality is None:
            return _degrade_u8(dev, patches, weights, sigma, seed, lr_sz, lr_sz)
        return _degrade_u8(dev, patches, weights, sigma, seed, lr_sz, lr_sz, quality, self.jpeg_subsampling, color)


BOX, BILINEAR = 4, 2     # PIL.Image.BOX / BILINEAR / srk_interp
USM_K, USM_WEIGHT, USM_THRESHOLD = 51, 0.5, 10.0   # Real-ESRGAN's USMSharp: radius 50 -> 51 taps, sigma 0 -> 8.0


def _usm(dev, patches):
    """USMSharp of dense 8-bit patches on the loader stream (srk_usm_u8); the Gaussian goes up once."""
    g = dev.resident_f64(("usm", USM_K), lambda: ops.usm_table(USM_K, 0.0))
    return dev.usm(patches, g, USM_WEIGHT, USM_THRESHOLD)


class Degradation2(object):
    """Real-ESRGAN's second-order degradation model on 8-bit stage boundaries.  Keywords carry
    Real-ESRGAN's names and defaults.  Per batch, [b] marking what is drawn per patch:

        stage 1: blur[b] -> resize to int(side * s1), filter of {BOX, BILINEAR, BICUBIC} -> noise[b] -> jpeg[b]
        stage 2: blur[b] (prob second_blur_prob) -> resize to int(lr side * s2) -> noise[b]
        final:   with prob 0.5  resize to the lr size -> sinc blur[b] (prob final_sinc_prob) -> jpeg[b]
                 else           jpeg[b] -> resize to the lr size -> sinc blur[b]
        lr = bytes / 255.0f

    Draws come from Python's global `random` (or the `rng` given to apply), after the batch's patch draws, in this order:
      1. stage-1 kernel of every patch (kernel(): below);
      2. stage-1 resize: random() against resize_prob -> up: uniform(1, hi) | down: uniform(lo, 1) | keep: no draw; then
         choice of the filter;
      3. stage-1 noise: random() < gaussian_noise_prob (Gaussian, else Poisson; once a batch); per patch uniform(amount
         range) then random() < gray_noise_prob; then getrandbits(64), the stage's seed;
      4. stage-1 JPEG quality of every patch: randint(lo, hi);
      5. per patch random() < second_blur_prob -> kernel(), else the delta;
      6. stage-2 resize as 2 (resize_prob2, resize_range2);  7. stage-2 noise as 3 (noise_range2, poisson_scale_range2);
      8. random() < 0.5: the final order;  9. choice of the final resize's filter;
      10. per patch random() < final_sinc_prob -> choice of K, uniform cutoff -> sinc table, else the delta;
      11. final JPEG quality of every patch: randint(lo, hi).
    kernel(): choice of K among kernel_sizes; random() < sinc_prob -> uniform cutoff ((pi / 3, pi) for K < 13, else
    (pi / 5, pi)); else random() against kernel_prob (iso, aniso, generalized iso, generalized aniso, plateau iso, plateau
    aniso) -> uniform s1; aniso: uniform s2, uniform(-pi, pi) theta; generalized: uniform beta of betag_range; plateau:
    of betap_range.  Nothing else is kept between batches, so a restored `random` state reproduces them."""

    DEFAULTS = dict(kernel_sizes=tuple(range(7, 22, 2)), kernel_sizes2=tuple(range(7, 22, 2)),
                    kernel_prob=(.45, .25, .12, .03, .12, .03), kernel_prob2=(.45, .25, .12, .03, .12, .03),
                    sinc_prob=.1, sinc_prob2=.1, blur_sigma=(0.2, 3.0), blur_sigma2=(0.2, 1.5),
                    betag_range=(0.5, 4.0), betag_range2=(0.5, 4.0), betap_range=(1.0, 2.0), betap_range2=(1.0, 2.0),
                    second_blur_prob=0.8, resize_prob=(.2, .7, .1), resize_prob2=(.3, .4, .3),
                    resize_range=(0.15, 1.5), resize_range2=(0.3, 1.2), gaussian_noise_prob=.5, gaussian_noise_prob2=.5,
                    noise_range=(1.0, 30.0), noise_range2=(1.0, 25.0), poisson_scale_range=(0.05, 3.0),
                    poisson_scale_range2=(0.05, 2.5), gray_noise_prob=.4, gray_noise_prob2=.4, jpeg_range=(30, 95),
                    jpeg_range2=(30, 95), final_sinc_prob=0.8, jpeg_subsampling='4:2:0')
    KINDS = (("gauss", False), ("gauss", True), ("ggauss", False), ("ggauss", True), ("plateau", False), ("plateau", True))
    FILTERS = (BOX, BILINEAR, BICUBIC)

    def __init__(self, **kw):
        unknown = sorted(set(kw) - set(self.DEFAULTS))
        if unknown:
            raise ValueError("Degradation2: unknown setting%s %s (known: %s)"
                             % ("s" if len(unknown) > 1 else "", ", ".join(unknown), ", ".join(sorted(self.DEFAULTS))))
        for name, dflt in self.DEFAULTS.items():
            v = kw.get(name, dflt)
            if name == 'jpeg_subsampling':
                self.jpeg_subsampling = jpeg_subsampling_code(v)
                continue
            if name.startswith('kernel_sizes'):
                v = tuple(int(k) for k in v)
                if not v or any(k % 2 == 0 or not 7 <= k <= BLUR_MAX_K for k in v):
                    raise ValueError("%s must be odd sizes in 7..%d (got %r)" % (name, BLUR_MAX_K, kw.get(name)))
            elif name.startswith('kernel_prob') or name.startswith('resize_prob'):
                v = tuple(float(x) for x in v)
                if len(v) != len(dflt) or min(v) < 0 or abs(sum(v) - 1.0) > 1e-9:
                    raise ValueError("%s must be %d probabilities that sum to 1 (got %r)" % (name, len(dflt), kw.get(name)))
            elif name.startswith('jpeg_range'):
                if len(v) != 2:
                    raise ValueError("%s must be (lo, hi) (got %r)" % (name, v))
                v = tuple(_check_jpeg_quality(q, "%s's bounds" % name) for q in v)
                if v[0] > v[1]:
                    raise ValueError("%s must be lo <= hi (got %r)" % (name, kw.get(name)))
            elif isinstance(dflt, tuple):
                v = tuple(float(x) for x in v)
                if len(v) != 2 or not 0.0 < v[0] <= v[1] < float('inf'):
                    raise ValueError("%s must be 0 < lo <= hi (got %r)" % (name, kw.get(name)))
            else:
                v = float(v)
                if not 0.0 <= v <= 1.0:
                    raise ValueError("%s must lie in [0, 1] (got %r)" % (name, kw.get(name)))
            setattr(self, name, v)
        for name in ('resize_range', 'resize_range2'):
            lo, hi = getattr(self, name)
            if not lo <= 1.0 <= hi:
                raise ValueError("%s must be lo <= 1 <= hi (got %r)" % (name, getattr(self, name)))

    def check(self, crop, sf):
        """Refuse a crop / scale at which a blurred side could not mirror the widest table's halo (reflect-101 with K = 21
        needs sides > 10): the stage-2 blur runs at int(crop * s1), the final one at crop // sf."""
        if min(int(crop * self.resize_range[0]), crop // sf) <= BLUR_MAX_K // 2:
            raise ValueError("resize_range %r with crop_size %d and scale_factor %d: the chain blurs sides of "
                             "int(crop_size * resize_range[0]) = %d and crop_size // scale_factor = %d, and both must exceed "
                             "%d (raise crop_size or resize_range's lower bound)"
                             % (self.resize_range, crop, sf, int(crop * self.resize_range[0]), crop // sf, BLUR_MAX_K // 2))

    # -- draws ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _cutoff(rng, K):
        return rng.uniform(math.pi / 3 if K < 13 else math.pi / 5, math.pi)

    def _kernel(self, rng, stage2):
        sfx = '2' if stage2 else ''
        K = rng.choice(getattr(self, 'kernel_sizes' + sfx))
        if rng.random() < getattr(self, 'sinc_prob' + sfx):
            return ops.blur_table("sinc", K, cutoff=self._cutoff(rng, K))
        r, acc, kind = rng.random(), 0.0, len(self.KINDS) - 1
        for i, pk in enumerate(getattr(self, 'kernel_prob' + sfx)):
            acc += pk
            if r < acc:
                kind = i
                break
        name, aniso = self.KINDS[kind]
        lo, hi = getattr(self, 'blur_sigma' + sfx)
        s1 = rng.uniform(lo, hi)
        s2, theta = (rng.uniform(lo, hi), rng.uniform(-math.pi, math.pi)) if aniso else (s1, 0.0)
        beta = 1.0
        if name == "ggauss":
            beta = rng.uniform(*getattr(self, 'betag_range' + sfx))
        elif name == "plateau":
            beta = rng.uniform(*getattr(self, 'betap_range' + sfx))
        return ops.blur_table(name, K, s1, s2, theta, beta)

    def _resize(self, rng, stage2):
        sfx = '2' if stage2 else ''
        up, down, _ = getattr(self, 'resize_prob' + sfx)
        lo, hi = getattr(self, 'resize_range' + sfx)
        r = rng.random()
        s = rng.uniform(1.0, hi) if r < up else (rng.uniform(lo, 1.0) if r < up + down else 1.0)
        return s, rng.choice(self.FILTERS)

    def _noise(self, rng, batch, stage2):
        sfx = '2' if stage2 else ''
        gauss = rng.random() < getattr(self, 'gaussian_noise_prob' + sfx)
        lo, hi = getattr(self, ('noise_range' if gauss else 'poisson_scale_range') + sfx)
        amount, gray = np.zeros(batch, np.float64), np.zeros(batch, np.float64)
        for j in range(batch):
            amount[j] = rng.uniform(lo, hi)
            gray[j] = float(rng.random() < getattr(self, 'gray_noise_prob' + sfx))
        mode = np.full(batch, float(ops.NOISE2_GAUSS if gauss else ops.NOISE2_POISSON), np.float64)
        return dict(mode=mode, gray=gray, amount=amount, seed=rng.getrandbits(64))

    def draw(self, batch, rng=random):
        """One batch's parameters as host values, in the order the class docstring fixes: a dict with the tables
        k1, k2, k3 [B, K, K] (narrower ones and the delta centred among zeros), the scales and filters s1, f1, s2, f2, f3,
        the noise dicts n1, n2 (mode, gray, amount [B], seed), the qualities q1, q2 [B] and `resize_first`."""
        p = {}
        t1 = [self._kernel(rng, False) for _ in range(batch)]
        p['s1'], p['f1'] = self._resize(rng, False)
        p['n1'] = self._noise(rng, batch, False)
        p['q1'] = np.array([rng.randint(*self.jpeg_range) for _ in range(batch)], np.float64)
        t2 = [self._kernel(rng, True) if rng.random() < self.second_blur_prob else None for _ in range(batch)]
        p['s2'], p['f2'] = self._resize(rng, True)
        p['n2'] = self._noise(rng, batch, True)
        p['resize_first'] = rng.random() < 0.5
        p['f3'] = rng.choice(self.FILTERS)
        t3 = []
        for _ in range(batch):
            if rng.random() < self.final_sinc_prob:
                K = rng.choice(self.kernel_sizes2)
                t3.append(ops.blur_table("sinc", K, cutoff=self._cutoff(rng, K)))
            else:
                t3.append(None)
        p['q2'] = np.array([rng.randint(*self.jpeg_range2) for _ in range(batch)], np.float64)
        for name, tables in (('k1', t1), ('k2', t2), ('k3', t3)):
            p[name] = _centred(tables, max([w.shape[0] for w in tables if w is not None] + [7]))
        return p

    def apply(self, dev, patches, lr_sz, color=True, rng=random):
        """Dense 8-bit patches [B, C, H, W] on the device -> the degraded fp32 lr [B, C, lr_sz, lr_sz] (lr_sz: a side, or
        (h, w)).  color: the planes are R, G, B (else Y, Cb, Cr): the JPEG stages and gray noise ask.  Every per-patch
        parameter and table crosses in one copy; a stage that is the identity for the whole batch (all-delta tables, an
        unchanged size, noise off, quality 0) is not launched."""
        b, c, h, w = (int(v) for v in patches.shape)
        lh, lw = (int(lr_sz), int(lr_sz)) if np.ndim(lr_sz) == 0 else (int(lr_sz[0]), int(lr_sz[1]))
        p = self.draw(b, rng)
        parts = [p['k1'], p['k2'], p['k3'], p['q1'], p['q2']] + [p[n][f] for n in ('n1', 'n2') for f in ('mode', 'gray', 'amount')]
        flat = dev.upload_f64(np.concatenate([a.reshape(-1) for a in parts]))
        on_dev, off = [], 0
        for a in parts:
            on_dev.append(flat[off:off + a.size].view(a.shape))
            off += a.size
        k1, k2, k3, q1, q2, m1, g1, a1, m2, g2, a2 = on_dev
        cdf = dev.resident_f64(("poisson", ops.POISSON_PEAK), ops.poisson_cdf)
        st = {'x': patches, 'h': h, 'w': w}

        def blur(host, table):
            K = host.shape[-1]
            if bool((host[:, K // 2, K // 2] != 1.0).any()):
                st['x'] = dev.blur(st['x'], table, c, b, st['h'], st['w'])

        def resize(oh, ow, filt, out_float=False):
            oh, ow = max(1, oh), max(1, ow)
            if (oh, ow) != (st['h'], st['w']) or out_float:
                st['x'] = dev.resize(st['x'], _CHW(st['h'], st['w']), b * c, st['h'], st['w'], oh, ow, out_float,
                                     filt=filt).view(b, c, oh, ow)
                st['h'], st['w'] = oh, ow

        def noise(n, mode, gray, amount, stage):
            if bool((n['mode'] != 0.0).any()):
                st['x'] = dev.noise2(st['x'], mode, gray, amount, cdf, n['seed'], stage, color)

        def jpeg(host, quality, out_float=False):
            if bool((host != 0.0).any()) or out_float:
                st['x'] = dev.jpeg(st['x'], quality, self.jpeg_subsampling, color, out_float=out_float)

        blur(p['k1'], k1)
        resize(int(h * p['s1']), int(w * p['s1']), p['f1'])
        noise(p['n1'], m1, g1, a1, 1)
        jpeg(p['q1'], q1)
        blur(p['k2'], k2)
        resize(int(lh * p['s2']), int(lw * p['s2']), p['f2'])
        noise(p['n2'], m2, g2, a2, 2)
        if p['resize_first']:
            resize(lh, lw, p['f3'])
            blur(p['k3'], k3)
            jpeg(p['q2'], q2, out_float=True)
        else:
            jpeg(p['q2'], q2)
            K = p['k3'].shape[-1]
            sinc = bool((p['k3'][:, K // 2, K // 2] != 1.0).any())
            resize(lh, lw, p['f3'], out_float=not sinc)
            if sinc:
                blur(p['k3'], k3)
                resize(lh, lw, p['f3'], out_float=True)      # (an unchanged size: the bytes / 255 and nothing else)
        return st['x']


class TrainDatasetFromFolder(object):
    """dataset.py:22-104 with device-side transforms.  `__getitem__` returns (lr_img, hr_img, bc_img) CUDA tensors."""

    def __init__(self, image_dirs, is_gray=False, random_scale=True, crop_size=128, rotate=True, fliplr=True,
                 fliptb=True, scale_factor=4, device="cuda", degrade=None, usm=False):
        self.image_filenames = []
        self.degrade = degrade    # a Degradation or a Degradation2, or None: the clean bicubic shrink of the reference
        self.usm = bool(usm)      # Real-ESRGAN's USMSharp on the 8-bit patches: hr and the shrink's input are the sharpened bytes
        if isinstance(degrade, Degradation2):
            degrade.check(calculate_valid_crop_size(crop_size, scale_factor), scale_factor)
        if self.usm and calculate_valid_crop_size(crop_size, scale_factor) <= USM_K // 2:
            raise ValueError("usm: crop_size %d must exceed %d, the radius of USMSharp's %d-tap Gaussian"
                             % (crop_size, USM_K // 2, USM_K))
        for image_dir in image_dirs:
            self.image_filenames.extend(join(image_dir, x) for x in sorted(listdir(image_dir)) if is_image_file(x))
        self.is_gray, self.random_scale, self.crop_size = is_gray, random_scale, crop_size
        self.rotate, self.fliplr, self.fliptb, self.scale_factor = rotate, fliplr, fliptb, scale_factor
        self._device, self._dev = device, None
        # Decoded images stay RESIDENT IN HBM as 8-bit tensors once they have been uploaded (DIV2K's 800 LR training images
        # are ~0.4 GB of 288): from the second epoch on a patch costs no PNG decode, no PCIe copy and one kernel call.  The
        # transforms still start from the same 8-bit pixels, so nothing changes numerically.  `resident_bytes` bounds it.
        self.resident_bytes = int(float(os.environ.get("SRK_DATA_RESIDENT_GB", "16")) * (1 << 30))
        self._resident, self._resident_used = {}, 0

    @property
    def dev(self):
        if self._dev is None:   # (created on first use: listing a folder and drawing parameters need no GPU)
            self._dev = _Device(self._device)
        return self._dev

    def __len__(self):
        return len(self.image_filenames)

    # -- the reference's random draws, in its order (dataset.py:51-82) -----------------------------------------
    def draw(self, w, h):
        """Consumes Python's `random` exactly like the reference's __getitem__ for a w x h image.  Returns
        (scale_wh or None, (x0, y0), rot_k, fliplr, fliptb)."""
        self.crop_size = calculate_valid_crop_size(self.crop_size, self.scale_factor)
        crop = self.crop_size
        scale = None
        if self.random_scale:
            eps = 1e-3
            ratio = random.randint(5, 10) * 0.1
            if crop * ratio < crop:
                ratio = crop / crop + eps
            if crop * ratio < crop:       # (second test of the reference, on the height: same numbers)
                ratio = crop / crop + eps
            scale = (int(crop * ratio), int(crop * ratio))
            w, h = scale
        x0 = y0 = 0
        if not (w == crop and h == crop):   # torchvision RandomCrop: no draw when the sizes already match
            if w < crop or h < crop:
                raise ValueError("image %dx%d is smaller than the crop size %d" % (w, h, crop))
            y0 = random.randint(0, h - crop)
            x0 = random.randint(0, w - crop)
        rot = random.randint(1, 3) if self.rotate else 0
        fl = (random.random() < 0.5) if self.fliplr else False
        ft = (random.random() < 0.5) if self.fliptb else False
        return scale, (x0, y0), rot, fl, ft

    def patch_u8(self, hwc, params, out=None):
        """Decoded image (numpy HWC uint8) + draws -> augmented 8-bit patch [3, crop, crop] on the device."""
        dev, crop = self.dev, self.crop_size
        scale, (x0, y0), rot, fl, ft = params
        if isinstance(hwc, torch.Tensor):    # resident image (see __init__)
            img = hwc
            h, w, c = img.shape
        else:
            h, w, c = hwc.shape
            img = dev.upload(hwc)
        if not self.is_gray:   # rescale + crop / rotation / flips in ONE call, straight into the batch buffer
            return dev.patch(img, c, h, w, scale, (x0, y0, crop, crop), rot, fl, ft, out)
        strides = _HWC(h, w, c)
        if scale is not None:
            img = dev.resize(img, strides, c, h, w, scale[1], scale[0], out_float=False)
            h, w = scale[1], scale[0]
            strides = _CHW(h, w)
        patch = dev.augment(img, strides, c, h, w, (x0, y0, crop, crop), rot, fl, ft, out=out)
        if self.is_gray:   # Pillow's integer RGB -> YCbCr matrix on the host (see module docstring)
            from PIL import Image
            with torch.cuda.stream(dev.stream):
                host = patch.permute(1, 2, 0).contiguous().cpu().numpy()
            ycc = np.asarray(Image.fromarray(host, "RGB").convert("YCbCr"), dtype=np.uint8)
            with torch.cuda.stream(dev.stream):
                patch.copy_(dev.upload(ycc).permute(2, 0, 1))
        return patch

    def resident(self, index):
        """The image's 8-bit device tensor if it is resident, else None."""
        return self._resident.get(index)

    def keep_resident(self, index, hwc):
        """Upload a decoded image and keep it in HBM (within the byte budget); returns what patch_u8 should consume."""
        n = int(hwc.size)
        if self._resident_used + n > self.resident_bytes:
            return hwc
        img = self.dev.upload(hwc)
        self._resident[index] = img
        self._resident_used += n
        return img

    def finish(self, patches):
        """[B, 3, crop, crop] 8-bit patches -> (lr, hr, bc) float batches: the three resizes of dataset.py:89-99."""
        dev, crop, sf = self.dev, self.crop_size, self.scale_factor
        b, c = patches.shape[0], patches.shape[1]
        lr_sz = crop // sf
        st = _CHW(crop, crop)
        if self.usm:
            patches = _usm(dev, patches.contiguous())
        hr = dev.resize(patches, st, b * c, crop, crop, crop, crop, out_float=True).view(b, c, crop, crop)
        if self.degrade is not None:
            lr = self.degrade.apply(dev, patches.contiguous(), lr_sz, color=not self.is_gray)
        else:
            lr = dev.resize(patches, st, b * c, crop, crop, lr_sz, lr_sz, out_float=True).view(b, c, lr_sz, lr_sz)
        bc = dev.bicubic_of_lr(lr, crop, crop)
        return lr, hr, bc

    def __getitem__(self, index):
        hwc = self.resident(index)
        if hwc is None:
            hwc = self.keep_resident(index, load_img(self.image_filenames[index]))
        params = self.draw(hwc.shape[1], hwc.shape[0])
        patch = self.patch_u8(hwc, params)
        lr, hr, bc = self.finish(patch.unsqueeze(0))
        return self.dev.hand_over(lr[0], hr[0], bc[0])


class TestDatasetFromFolder(object):
    """dataset.py:106-149 with device-side resizes."""

    def __init__(self, image_dir, is_gray=False, scale_factor=4, device="cuda", degrade=None, jpeg=None,
                 jpeg_subsampling='4:2:0', degrade2=None):
        self.image_filenames = [join(image_dir, x) for x in sorted(listdir(image_dir)) if is_image_file(x)]
        # degrade2: None, or (Degradation2, seed): item i's whole chain is drawn from a private random.Random seeded by
        # (seed, i), so an item is the same on every read and the global `random` is left alone
        self.degrade2 = None
        if degrade2 is not None:
            if degrade is not None or jpeg is not None:
                raise ValueError("degrade2 brings its own blur, noise and JPEG stages: give neither degrade nor jpeg with it")
            if not (len(degrade2) == 2 and isinstance(degrade2[0], Degradation2)):
                raise ValueError("degrade2 must be (Degradation2, seed), got %r" % (degrade2,))
            self.degrade2 = (degrade2[0], int(degrade2[1]))
        # jpeg: None, or one FIXED quality 1..100 at which every low-resolution image is compressed and decoded again,
        # behind the degradation where there is one
        self.jpeg = None if jpeg is None else _check_jpeg_quality(jpeg, "jpeg")
        self.jpeg_subsampling = jpeg_subsampling_code(jpeg_subsampling)
        self.is_gray, self.scale_factor = is_gray, scale_factor
        # degrade: None, or one FIXED degradation (s1, s2, theta in radians, noise sigma in 8-bit levels) for every image,
        # the noise seeded with the image's index: an item is the same on every read
        self.degrade = None if degrade is None else tuple(float(v) for v in degrade)
        if self.degrade is not None and not (len(self.degrade) == 4 and self.degrade[0] > 0 and self.degrade[1] > 0
                                             and self.degrade[3] >= 0):
            raise ValueError("degrade must be (s1 > 0, s2 > 0, theta, noise_sigma >= 0), got %r" % (degrade,))
        self._device, self._dev = device, None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = _Device(self._device)
        return self._dev

    def __len__(self):
        return len(self.image_filenames)

    def __getitem__(self, index):
        from PIL import Image
        dev, sf = self.dev, self.scale_factor
        if self.is_gray:
            hwc = np.asarray(Image.open(self.image_filenames[index]).convert('RGB').convert('YCbCr'), dtype=np.uint8)
        else:
            hwc = load_img(self.image_filenames[index])
        h, w, c = hwc.shape
        hr_w, hr_h = calculate_valid_crop_size(w, sf), calculate_valid_crop_size(h, sf)
        lr_w, lr_h = hr_w // sf, hr_h // sf
        img = dev.upload(hwc)
        st = _HWC(h, w, c)
        hr = dev.resize(img, st, c, h, w, hr_h, hr_w, out_float=True)
        if self.degrade2 is not None:
            d, seed = self.degrade2
            if min(int(h * d.resize_range[0]), int(w * d.resize_range[0]), lr_h, lr_w) <= BLUR_MAX_K // 2:
                raise ValueError("degrade2: image %dx%d is too small for resize_range %r at scale_factor %d (every blurred "
                                 "side must exceed %d)" % (w, h, d.resize_range, sf, BLUR_MAX_K // 2))
            with torch.cuda.stream(dev.stream):
                planes = img.permute(2, 0, 1).contiguous().unsqueeze(0)
            lr = d.apply(dev, planes, (lr_h, lr_w), color=not self.is_gray, rng=test_item_rng(seed, index))[0]
        elif self.degrade is not None or self.jpeg is not None:
            with torch.cuda.stream(dev.stream):
                planes = img.permute(2, 0, 1).contiguous().unsqueeze(0)   # (the blur reads dense planes)
            if self.degrade is not None:
                s1, s2, theta, noise_sigma = self.degrade
                table = blur_weights(s1, s2, theta)[None]
            else:                                                         # a clean shrink, then JPEG
                noise_sigma, table = 0.0, _centred([None], 3)
            jpeg = () if self.jpeg is None else (np.array([self.jpeg], np.float64), self.jpeg_subsampling, not self.is_gray)
            lr = _degrade_u8(dev, planes, table, np.array([noise_sigma], np.float64), index, lr_h, lr_w, *jpeg)[0]
        else:
            lr = dev.resize(img, st, c, h, w, lr_h, lr_w, out_float=True)
        bc = dev.bicubic_of_lr(lr.unsqueeze(0), hr_h, hr_w)[0]
        return dev.hand_over(lr, hr, bc)


def test_item_rng(seed, index):
    """The private generator of test item `index` under degrade2's `seed`."""
    return random.Random("degrade2:%d:%d" % (int(seed), int(index)))


def get_training_set(data_dir, datasets, crop_size, scale_factor, is_gray=False, device="cuda", degrade=None, usm=False):
    """data.py:33-51 (directory layout and augmentation switches; 'bsds300' must already be on disk)."""
    train_dir = []
    for dataset in datasets:
        if dataset == 'bsds300':
            train_dir.append(join(data_dir, "BSDS300/images", "train"))
        elif dataset == 'DIV2K':
            train_dir.append(join(data_dir, dataset, 'DIV2K_train_LR_bicubic/X4'))
        else:
            train_dir.append(join(data_dir, dataset))
    return TrainDatasetFromFolder(train_dir, is_gray=is_gray, random_scale=True, crop_size=crop_size, rotate=True,
                                  fliplr=True, fliptb=True, scale_factor=scale_factor, device=device, degrade=degrade,
                                  usm=usm)


def get_test_set(data_dir, dataset, scale_factor, is_gray=False, device="cuda", degrade=None, jpeg=None,
                 jpeg_subsampling='4:2:0', degrade2=None):
    """data.py:54-65"""
    if dataset == 'bsds300':
        test_dir = join(data_dir, "BSDS300/images", "test")
    elif dataset == 'DIV2K':
        test_dir = join(data_dir, dataset, 'DIV2K_test_LR_bicubic/X4')
    else:
        test_dir = join(data_dir, dataset)
    return TestDatasetFromFolder(test_dir, is_gray=is_gray, scale_factor=scale_factor, device=device, degrade=degrade,
                                 jpeg=jpeg, jpeg_subsampling=jpeg_subsampling, degrade2=degrade2)


class ClipDataset(object):
    """Training clips for VESPCN: data_dir/<dataset>/<clip>/<frames>, the frames of a clip sorted by name.  An item is
    three consecutive frames of one clip; ONE draw (crop, rotation, flips; no random rescale) is applied to all three
    through the per-patch call of TrainDatasetFromFolder, whose Pillow-exact shrink makes the LR frames.  Returns
    (frames [3,C,lr,lr], the centre HR frame [C,crop,crop]) CUDA tensors.  The draws come from Python's `random`, so
    --resume reproduces them.  Runs through PatchLoader's per-item path (`decode_ahead = False`: the loader submits no file to its decode pool)."""

    def __init__(self, clip_root_dirs, is_gray=False, crop_size=128, scale_factor=4, device="cuda"):
        self.items = []          # (frame t-1, frame t, frame t+1) file names
        self.clips = []          # (clip directory, its frame files)
        for root in clip_root_dirs:
            for clip in sorted(listdir(root)):
                if not os.path.isdir(join(root, clip)):
                    continue
                frames = [join(root, clip, x) for x in sorted(listdir(join(root, clip))) if is_image_file(x)]
                self.clips.append((join(root, clip), frames))
                self.items.extend(tuple(frames[i:i + 3]) for i in range(len(frames) - 2))
        self.image_filenames = [it[1] for it in self.items]      # the centre frames (what PatchLoader would decode)
        self.patcher = TrainDatasetFromFolder([], is_gray=is_gray, random_scale=False, crop_size=crop_size, rotate=True,
                                              fliplr=True, fliptb=True, scale_factor=scale_factor, device=device)

    dev = property(lambda self: self.patcher.dev)
    decode_ahead = False      # PatchLoader: an item reads its own three files, there is no one file to decode ahead

    def __len__(self):
        return len(self.items)

    def __getitem__(self, index):
        p = self.patcher
        frames = [load_img(fn) for fn in self.items[index]]
        h, w = frames[1].shape[0], frames[1].shape[1]
        for fn, f in zip(self.items[index], frames):
            if f.shape[:2] != (h, w):
                raise ValueError("clip frame %s is %d x %d, its neighbour %d x %d" % (fn, f.shape[1], f.shape[0], w, h))
        params = p.draw(w, h)                                     # one draw for the three frames
        crop = p.crop_size                                        # (draw made it a multiple of the scale)
        with p.dev.batch():
            patches = torch.empty((3, 3, crop, crop), dtype=torch.uint8, device=p.dev.device)
            for j, f in enumerate(frames):
                p.patch_u8(f, params, out=patches[j])
            lr, hr, _ = p.finish(patches)
        return p.dev.hand_over(lr, hr[1])


class ClipTestDataset(object):
    """Test clips for VESPCN: data_dir/<dataset>/<clip>/<frames>.  Item t of a clip is (the LR frames t-1, t, t+1 of that
    clip as [3,C,h,w], the ends using themselves; the HR frame t), each frame made by TestDatasetFromFolder's item: every
    frame is evaluated once, with its real neighbours."""
    decode_ahead = False

    def __init__(self, root, is_gray=False, scale_factor=4, device="cuda"):
        self.clips = []
        for clip in sorted(listdir(root)):
            if os.path.isdir(join(root, clip)):
                ds = TestDatasetFromFolder(join(root, clip), is_gray=is_gray, scale_factor=scale_factor, device=device)
                if len(ds):
                    self.clips.append(ds)
        self.index = [(c, t) for c, ds in enumerate(self.clips) for t in range(len(ds))]
        self.image_filenames = [self.clips[c].image_filenames[t] for c, t in self.index]

    def __len__(self):
        return len(self.index)

    def neighbours(self, index):
        """(clip number, (t-1, t, t+1) clamped to the clip) of an item."""
        c, t = self.index[index]
        return c, (max(t - 1, 0), t, min(t + 1, len(self.clips[c]) - 1))

    def __getitem__(self, index):
        c, ts = self.neighbours(index)
        ds = self.clips[c]
        made = {t: ds[t] for t in sorted(set(ts))}
        lr = [made[t][0] for t in ts]
        if len(set(x.shape for x in lr)) != 1:
            raise ValueError("clip %s: frames of different sizes around %s" % (os.path.dirname(ds.image_filenames[0]),
                                                                              ds.image_filenames[ts[1]]))
        return torch.stack(lr), made[ts[1]][1]


def get_clip_test_set(data_dir, dataset, scale_factor, is_gray=False, device="cuda"):
    return ClipTestDataset(join(data_dir, dataset), is_gray=is_gray, scale_factor=scale_factor, device=device)


def get_clip_training_set(data_dir, datasets, crop_size, scale_factor, is_gray=False, device="cuda"):
    return ClipDataset([join(data_dir, d) for d in datasets], is_gray=is_gray, crop_size=crop_size,
                       scale_factor=scale_factor, device=device)


class PatchLoader(object):
    """DataLoader(dataset=train_set, num_workers=num_threads, batch_size=B, shuffle=True) of the reference
    (edsr.py:75-77), MI355X-first: `num_threads` host threads only DECODE (the next batch is decoded while the current
    one trains), pixels cross PCIe as uint8 through pinned memory, all transforms run on the loader's HIP stream, and a
    batch costs 2-3 small launches per patch plus three batched resizes.  Yields (lr, hr, bc) CUDA batches."""

    def __init__(self, dataset, batch_size, shuffle=True, num_threads=4, drop_last=False, seed=None, background=True,
                 rank=0, world=1):
        self.ds, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        # data parallel (world > 1): every rank draws the SAME permutation per epoch (so `seed` must be common; default
        # 0) and takes its own strided 1/world of it, wrapped around so that all ranks see the same number of batches
        self.rank, self.world = int(rank), max(1, int(world))
        if self.world > 1 and seed is None:
            seed = 0
        # background: batches are produced by a loader thread up to two ahead of the consumer (its host work -- draws,
        # one call per patch, three batched resizes -- overlaps with the consumer launching / replaying the train step)
        self.background = bool(background)
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(num_threads)))
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed))

    def state_dict(self):
        """What an epoch boundary leaves of the loader: the shuffle generator (the crops and flips draw from Python's
        global `random`, which whoever saves a training state saves with it).  Needs no GPU."""
        return {"gen": self.gen.get_state().clone()}

    def load_state_dict(self, sd):
        self.gen.set_state(sd["gen"])

    def _shard_len(self):
        return -(-len(self.ds) // self.world)      # ceil: short ranks wrap around (torch's DistributedSampler rule)

    def __len__(self):
        n = self._shard_len()
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _order(self):
        """This rank's image indices of one epoch."""
        n = len(self.ds)
        order = torch.randperm(n, generator=self.gen).tolist() if self.shuffle else list(range(n))
        if self.world > 1:
            per = self._shard_len()
            order = (order + order[:per * self.world - n])[self.rank:per * self.world:self.world]
        return order

    def _batches(self):
        order = self._order()
        n = len(order)
        for i in range(0, n, self.batch_size):
            idx = order[i:i + self.batch_size]
            if len(idx) < self.batch_size and self.drop_last:
                return
            yield idx

    def _decode(self, idx):
        if not getattr(self.ds, "decode_ahead", True):     # (clip datasets: an item reads its own files)
            return [(i, None) for i in idx]
        res = getattr(self.ds, "resident", None)
        return [(i, None if (res is not None and res(i) is not None) else self.pool.submit(load_img, self.ds.image_filenames[i]))
                for i in idx]

    def __iter__(self):
        ds = self.ds
        if not (self.background and isinstance(ds, TrainDatasetFromFolder)):
            for tensors, ev in self._produce():
                yield ds.dev.hand_over(*tensors) if ev is not None else tensors
            return
        import queue
        import threading
        q, stop, END = queue.Queue(maxsize=2), threading.Event(), object()

        def put(item):
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def work():
            try:
                for item in self._produce():
                    if not put(item):
                        return
                put(END)
            except BaseException as e:   # noqa: BLE001 -- re-raised in the consumer
                put(e)

        th = threading.Thread(target=work, name="srk-loader", daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is END:
                    break
                if isinstance(item, BaseException):
                    raise item
                tensors, ev = item
                cur = torch.cuda.current_stream(ds.dev.device)
                cur.wait_event(ev)            # the consumer's stream waits for THIS batch only, not for the loader stream
                for t in tensors:
                    t.record_stream(cur)
                yield tensors
        finally:
            stop.set()

    def _produce(self):
        """Generator of (batch tensors, event recorded on the loader stream behind them); event None = nothing to wait
        for (test items are handed over one by one)."""
        ds = self.ds
        batches = list(self._batches())
        # decode ahead: enough batches in flight to keep every decode thread busy while the current batch is uploaded
        # and transformed (one batch ahead leaves 32 threads half idle at batch 16: 2.6 k -> patches/s decode-bound)
        depth = max(1, -(-self.pool._max_workers // max(1, self.batch_size))) + 1
        from collections import deque
        pending = deque(self._decode(b) for b in batches[:depth])
        for k, idx in enumerate(batches):
            images = []
            for i, f in pending.popleft():
                if f is None:
                    images.append(ds.resident(i) if hasattr(ds, "resident") else None)
                elif isinstance(ds, TrainDatasetFromFolder):
                    with ds.dev.batch():
                        images.append(ds.keep_resident(i, f.result()))
                else:
                    images.append(f.result())
            if k + depth < len(batches):
                pending.append(self._decode(batches[k + depth]))   # overlaps with the work below
            if isinstance(ds, TrainDatasetFromFolder):
                crop = calculate_valid_crop_size(ds.crop_size, ds.scale_factor)
                with ds.dev.batch():
                    patches = torch.empty((len(idx), 3, crop, crop), dtype=torch.uint8, device=ds.dev.device)
                    for j, hwc in enumerate(images):
                        ds.patch_u8(hwc, ds.draw(hwc.shape[1], hwc.shape[0]), out=patches[j])
                    out = ds.finish(patches)
                    ev = torch.cuda.Event()
                    ev.record(ds.dev.stream)
                yield out, ev
            else:   # test images differ in size: one item per batch entry, stacked only when they agree
                items = [ds[i] for i in idx]
                yield tuple(torch.stack(t) if len(set(x.shape for x in t)) == 1 else list(t) for t in zip(*items)), None


# ------------------------------------------------------------------------------------------------
# YUV4MPEG2 (.y4m): raw planar 8-bit video behind text headers -- the container of test_video.  It needs no codec
# library, and `ffmpeg -f yuv4mpegpipe` reads and writes it through pipes.
#   stream:  "YUV4MPEG2 W.. H.. [F..] [I..] [A..] [C..] [X..]*\n", then per frame "FRAME[ params]\n" + the payload
#   payload: Y [H][W], then Cb and Cr (ops.yuv_layout is the one place that says where)
# ------------------------------------------------------------------------------------------------
Y4M_MAGIC = b"YUV4MPEG2"
Y4M_CHROMA = {"C420jpeg": "420", "C420mpeg2": "420", "C420paldv": "420", "C420": "420", "C444": "444", "Cmono": "mono"}
Y4M_INTERLACE = ("Ip", "I?")
_Y4M_LINE_LIMIT = 4096


class Y4MHeader(object):
    """The stream header: W, H and the other tags as they came, in their order.  A missing C tag means C420jpeg.
    Everything the kernels do not take is a ValueError that names the tag: 4:2:2, any depth above 8 bits, alpha,
    interlaced material, an unknown tag."""

    def __init__(self, tokens):
        self.tokens = list(tokens)
        self.W = self.H = None
        self.chroma_tag = None
        for t in self.tokens:
            if t[:1] == "W" or t[:1] == "H":
                if not t[1:].isdigit() or int(t[1:]) <= 0:
                    raise ValueError("Y4M header: bad size tag %r" % t)
                setattr(self, t[0], int(t[1:]))
            elif t[:1] == "C":
                if t not in Y4M_CHROMA:
                    raise ValueError("Y4M header: chroma tag %r is not supported (8-bit %s only)" % (t, ", ".join(sorted(Y4M_CHROMA))))
                self.chroma_tag = t
            elif t[:1] == "I":
                if t not in Y4M_INTERLACE:
                    raise ValueError("Y4M header: interlacing tag %r is not supported (progressive %s only)"
                                     % (t, " / ".join(Y4M_INTERLACE)))
            elif t[:1] not in ("F", "A", "X"):
                raise ValueError("Y4M header: unknown tag %r" % t)
        if self.W is None or self.H is None:
            raise ValueError("Y4M header: no %s tag" % ("W" if self.W is None else "H"))
        self.layout = ops.yuv_layout(self.W, self.H, Y4M_CHROMA[self.chroma_tag or "C420jpeg"], self.chroma_tag or "C420jpeg")

    @classmethod
    def parse(cls, line):
        if not line.endswith(b"\n"):
            raise ValueError("Y4M header: no end of line within %d bytes (got %r...)" % (len(line), line[:32]))
        parts = line[:-1].decode("ascii", "replace").split(" ")
        if parts[0] != Y4M_MAGIC.decode():
            raise ValueError("not a YUV4MPEG2 stream: it begins with %r" % line[:16])
        return cls([p for p in parts[1:] if p])

    def scaled(self, W, H):
        """The header of the super-resolved stream: W and H replaced, every other tag (F, I, A, C, X) carried through."""
        return Y4MHeader([("W%d" % W) if t[:1] == "W" else ("H%d" % H) if t[:1] == "H" else t for t in self.tokens])

    def line(self):
        return " ".join([Y4M_MAGIC.decode()] + self.tokens).encode("ascii") + b"\n"


def _y4m_open(target, mode):
    """(file object, whether we close it): a path, '-' (stdin / stdout, binary) or a binary file object."""
    if hasattr(target, "read" if mode == "rb" else "write"):
        return target, False
    if os.fspath(target) == "-":
        import sys
        return (sys.stdin if mode == "rb" else sys.stdout).buffer, False
    if mode == "wb" and os.path.dirname(os.fspath(target)):
        os.makedirs(os.path.dirname(os.fspath(target)), exist_ok=True)
    return open(target, mode), True


def _y4m_bytes(buf):
    """A writable flat byte view of a CPU uint8 tensor (pinned or not), a numpy array or any buffer object."""
    if torch.is_tensor(buf):
        if buf.dtype != torch.uint8 or buf.is_cuda or not buf.is_contiguous():
            raise ValueError("Y4M: a frame buffer must be a dense uint8 tensor on the host")
        buf = buf.numpy()
    return memoryview(buf).cast("B")


class Y4MReader(object):
    """Streams a YUV4MPEG2 source (a pipe has no length): read_into(buf, n) copies up to n frame payloads straight into the
    caller's buffer -- dense, frame k at byte k * layout.frame_bytes, so frames start at any alignment -- and returns how
    many came (0: the stream has ended).  batches(buffers, n) walks the whole stream through rotating buffers."""

    def __init__(self, src):
        self.f, self._own = _y4m_open(src, "rb")
        try:
            self.header = Y4MHeader.parse(self.f.readline(_Y4M_LINE_LIMIT))
        except Exception:
            self.close()
            raise
        self.layout = self.header.layout
        self.frames_read = 0

    def _fill(self, view):
        got = 0
        readinto = getattr(self.f, "readinto", None)
        while got < len(view):
            if readinto is not None:
                k = readinto(view[got:])
            else:
                chunk = self.f.read(len(view) - got)
                k = len(chunk)
                view[got:got + k] = chunk
            if not k:
                break
            got += k
        return got

    def read_into(self, buf, max_frames=None):
        view = _y4m_bytes(buf)
        fb = self.layout.frame_bytes
        room = len(view) // fb
        n = room if max_frames is None else min(int(max_frames), room)
        if n <= 0:
            raise ValueError("Y4M: a buffer of %d bytes holds no frame of %d bytes" % (len(view), fb))
        for k in range(n):
            line = self.f.readline(_Y4M_LINE_LIMIT)
            if not line:
                return k
            if line[:5] != b"FRAME" or line[5:6] not in (b" ", b"\n") or not line.endswith(b"\n"):
                raise ValueError("Y4M: frame %d does not begin with a FRAME line (got %r)" % (self.frames_read, line[:16]))
            got = self._fill(view[k * fb:(k + 1) * fb])
            if got != fb:
                raise ValueError("Y4M: frame %d ends early: got %d bytes, expected %d" % (self.frames_read, got, fb))
            self.frames_read += 1
        return n

    def batches(self, buffers, n):
        """Yields (buffer, frames) over the whole stream; the buffers rotate, so a yielded one is overwritten len(buffers)
        batches later."""
        i = 0
        while True:
            k = self.read_into(buffers[i % len(buffers)], n)
            if k == 0:
                return
            yield buffers[i % len(buffers)], k
            i += 1
            if k < n:
                return

    def close(self):
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter(object):
    """Writes `header` (a Y4MHeader; Y4MHeader.scaled makes the output side's), then per frame a bare "FRAME\\n" and the
    payload.  write(buf, n) takes n dense frames from a buffer as Y4MReader.read_into fills it."""

    def __init__(self, dst, header):
        self.header, self.layout = header, header.layout
        self.f, self._own = _y4m_open(dst, "wb")
        self.f.write(header.line())
        self.frames_written = 0

    def write(self, buf, n=None):
        view = _y4m_bytes(buf)
        fb = self.layout.frame_bytes
        n = len(view) // fb if n is None else int(n)
        if n * fb > len(view):
            raise ValueError("Y4M: %d frames of %d bytes do not fit a buffer of %d bytes" % (n, fb, len(view)))
        for k in range(n):
            self.f.write(b"FRAME\n")
            self.f.write(view[k * fb:(k + 1) * fb])
        self.frames_written += n

    def close(self):
        self.f.flush()
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
