"""The colour tail without a GPU: the library's RGB <-> YCbCr tables against Pillow on every 24-bit input (the host
helpers read the very tables the kernels get), and the command line of the single-image entry."""
import ctypes
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def every_triple():
    """The 4096 x 4096 x 3 image that holds every 8-bit triple once: pixel i = (i >> 16, (i >> 8) & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8)
    return np.ascontiguousarray(img.reshape(4096, 4096, 3))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import _lib
    return _lib.load()


def _host(fn, img):
    out = np.empty_like(img)
    rc = fn(ctypes.c_void_p(img.ctypes.data), img.shape[0] * img.shape[1], ctypes.c_void_p(out.ctypes.data))
    assert rc == 0
    return out


def test_rgb_to_ycc_host_equals_pillow_on_every_rgb_triple(lib):
    img = every_triple()
    ref = np.asarray(Image.fromarray(img, "RGB").convert("YCbCr"))
    got = _host(lib.srk_rgb_to_ycc_host, img)
    bad = int((got != ref).any(axis=-1).sum())
    assert np.array_equal(got, ref), "%d of 2^24 triples differ" % bad


def test_ycc_to_rgb_host_equals_pillow_on_every_ycc_triple(lib):
    img = every_triple()
    ref = np.asarray(Image.fromarray(img, "YCbCr").convert("RGB"))
    got = _host(lib.srk_ycc_to_rgb_host, img)
    bad = int((got != ref).any(axis=-1).sum())
    assert np.array_equal(got, ref), "%d of 2^24 triples differ" % bad


def test_host_helpers_reject_null_pointers(lib):
    buf = np.zeros(3, np.uint8)
    assert lib.srk_rgb_to_ycc_host(None, 1, ctypes.c_void_p(buf.ctypes.data)) == -1
    assert lib.srk_ycc_to_rgb_host(ctypes.c_void_p(buf.ctypes.data), 1, None) == -1
    assert lib.srk_rgb_to_ycc_host(None, 0, None) == -1


def test_device_entry_points_check_arguments_before_any_launch(lib):
    """Bad arguments fail in SRK_REQUIRE, before a stream is touched: this runs on a machine without a GPU."""
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below is rejected first
    assert lib.srk_rgb_to_ycc_u8(None, 48, 4, 16, p, None, None, None) == -1
    assert lib.srk_rgb_to_ycc_u8(p, 48, 0, 16, p, None, None, None) == -1
    assert lib.srk_rgb_to_ycc_u8(p, 47, 4, 16, p, None, None, None) == -1       # row stride < 3 W
    assert lib.srk_rgb_to_ycc_u8(p, 48, 4, 16, None, None, None, None) == -1    # no output asked for
    assert lib.srk_ycc_to_rgb_u8(p, 16, 1, p, p, p, p, 4, 16, None) == -1       # both forms of Y
    assert lib.srk_ycc_to_rgb_u8(None, 0, 0, None, p, p, p, 4, 16, None) == -1  # no Y
    assert lib.srk_ycc_to_rgb_u8(None, 0, 0, p, p, None, p, 4, 16, None) == -1
    assert lib.srk_ycc_to_rgb_u8(p, -16, 1, None, p, p, p, 4, 16, None) == -1
    assert lib.srk_float_to_u8_image(p, 64, 16, 1, p, 2, 4, 16, None) == -1     # C must be 1 or 3
    assert lib.srk_float_to_u8_image(p, 64, 16, 1, None, 3, 4, 16, None) == -1
    assert lib.srk_float_to_u8_image(p, 64, 16, 1, p, 3, 4, -1, None) == -1
    assert b"float_to_u8_image" in lib.srk_last_error_string()


def test_cli_carries_the_single_image_path(tmp_path):
    import main as cli
    a = cli.parse_args(["--model_name", "VDSR", "--num_channels", "1", "--test_single", "x.png", "--save_dir", str(tmp_path)])
    assert a.test_single == "x.png" and a.save_test_images is False
    b = cli.parse_args(["--save_dir", str(tmp_path), "--save_test_images"])
    assert b.test_single is None and b.save_test_images is True
    c = cli.parse_args(["--save_dir", str(tmp_path)])
    assert c.test_single is None and c.save_test_images is False
    assert (c.model_name, c.num_channels, c.scale_factor, c.precision) == ("SRGAN", 3, 4, "mixed")


def test_save_img_file_names_follow_the_reference():
    from pytorch_super_resolution_model_collection_amd import utils
    assert utils.save_img_name(7, "d") == "d/SR_result_7.png"
    assert utils.save_img_name(3, "d", is_training=True) == "d/SR_result_epoch_3.png"
