"""CPU (-m "not gpu"): the arithmetic of the device image preparation, pinned without a GPU.  The numpy restatement
(tests/image_prep_ref.py) equals the fixtures produced by the reference (tests/golden/make_golden_image_prep.py) and equals PIL directly,
bit for bit; the host-side pieces of mindtheedge_amd/datasets/image_prep.py (coefficient tables, jitter draws, crop borders, config
defaults) equal the restatement / the reference's recorded results."""
import json
import os
import random

import numpy as np
import pytest
from PIL import Image, ImageEnhance

import image_prep_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep.npz")
RESIZES = [((375, 1242), (384, 1280), None), ((370, 1226), (384, 1280), None), ((97, 131), (64, 192), None), ((50, 70), (120, 33), None),
           ((64, 64), (64, 100), None), ((97, 131), (64, 192), (7, 10, 107, 70)), ((1, 1), (5, 4), None), ((40, 7), (13, 3), None)]


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def test_resize_equals_reference_fixtures(z):
    for name in ("rand", "smooth", "mixed", "skip"):
        got = R.resize_u8(z["resize_%s_in" % name], tuple(int(v) for v in z["resize_%s_shape" % name]))
        np.testing.assert_array_equal(got, z["resize_%s_out" % name])
    for i in range(3):
        b = tuple(int(v) for v in z["crop%d_borders" % i])
        np.testing.assert_array_equal(z["resize_rand_in"][b[1]:b[3], b[0]:b[2]], z["crop%d_rgb" % i])
        np.testing.assert_array_equal(R.resize_u8(z["resize_rand_in"], (64, 192), crop=b), z["crop%d_rgb_resized" % i])
        np.testing.assert_array_equal(z["crop_depth_in"][b[1]:b[3], b[0]:b[2]], z["crop%d_depth" % i])
        np.testing.assert_array_equal(z["crop_edge_in"][b[1]:b[3], b[0]:b[2]], z["crop%d_edge" % i])


@pytest.mark.parametrize("src,dst,crop", RESIZES)
def test_resize_equals_pil(src, dst, crop):
    img = np.random.default_rng(src[0] * 7 + dst[1]).integers(0, 256, src + (3,), dtype=np.uint8)
    p = Image.fromarray(img)
    if crop is not None:
        p = p.crop(crop)
    np.testing.assert_array_equal(R.resize_u8(img, dst, crop), np.asarray(p.resize(dst[::-1], Image.LANCZOS)))


def test_enhance_operations_equal_pil_over_a_factor_sweep():
    img = np.random.default_rng(3).integers(0, 256, (61, 67, 3), dtype=np.uint8)
    img[:8] = 255
    img[8:16] = 0
    p = Image.fromarray(img)
    for f in (0, 0.5, 0.8, 0.8134, 0.9999, 1.0, 1.0001, 1.1999, 1.2, 1.7, 3.0):
        np.testing.assert_array_equal(R.adjust_brightness(img, f), np.asarray(ImageEnhance.Brightness(p).enhance(f)))
        np.testing.assert_array_equal(R.adjust_contrast(img, f), np.asarray(ImageEnhance.Contrast(p).enhance(f)))
        np.testing.assert_array_equal(R.adjust_saturation(img, f), np.asarray(ImageEnhance.Color(p).enhance(f)))


def test_hsv_conversions_equal_pil_over_all_colours():
    a = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    np.testing.assert_array_equal(R.rgb_to_hsv(cube), np.asarray(Image.fromarray(cube, "RGB").convert("HSV")))
    np.testing.assert_array_equal(R.hsv_to_rgb(cube), np.asarray(Image.frombytes("HSV", (4096, 4096), cube.tobytes()).convert("RGB")))


def test_jitter_equals_reference_fixtures_and_draws(z):
    from mindtheedge_amd.datasets.image_prep import draw_color_jitter
    params = tuple(float(v) for v in z["jitter_params"])
    positions = set()
    for i, k in enumerate(int(v) for v in z["jitter_seeds"]):
        random.seed(k)
        drawn = draw_color_jitter(params)
        assert drawn["factors"] == tuple(z["jitter_factors"][i]) and drawn["order"] == tuple(z["jitter_orders"][i])
        positions.add(drawn["order"].index(1))
        for name in ("rand", "smooth"):
            got = R.color_jitter(z["jitter_%s_in" % name], drawn["factors"], drawn["order"])
            np.testing.assert_array_equal(got, z["jitter_%s_seed%d" % (name, k)])
        if k < 4:
            np.testing.assert_array_equal(R.to_tensor(R.color_jitter(z["jitter_rand_in"], drawn["factors"], drawn["order"])),
                                          z["jitter_rand_seed%d_tensor" % k])
    assert positions == {0, 1, 2, 3}                                         # contrast first, in the middle and last are all covered
    for name in ("rand", "smooth"):
        np.testing.assert_array_equal(R.to_tensor(z["jitter_%s_in" % name]), z["jitter_%s_tensor" % name])
    # a second draw continues the stream like the reference's next sample; () draws nothing; the colour matrix is not rebuilt
    random.seed(5)
    a, b = draw_color_jitter(params), draw_color_jitter(params)
    assert a != b
    state = random.getstate()
    assert draw_color_jitter(()) is None and random.getstate() == state
    with pytest.raises(NotImplementedError):
        draw_color_jitter((0.2, 0.2, 0.2, 0.05, 0.1))
    assert draw_color_jitter((0.2, 0.2, 0.2, 0.05, 0.0)) is not None


def test_hue_wrapper_roundtrip_against_pil():
    img = np.random.default_rng(4).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    for f in (0.0, 0.05, -0.05, 0.0123, -0.5, 0.5):
        h, s, v = Image.fromarray(img).convert("HSV").split()
        nh = ((np.array(h, dtype=np.int32) + int(f * 255) % 256) % 256).astype(np.uint8)
        want = np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
        np.testing.assert_array_equal(R.adjust_hue(img, f), want)


def test_parse_crop_borders_equals_reference_cases(z):
    from mindtheedge_amd.datasets.image_prep import parse_crop_borders
    cases = json.loads(str(z["crop_cases"]))
    assert len(cases) >= 9
    for c in cases:
        assert list(parse_crop_borders(tuple(c["borders"]), tuple(c["shape"]))) == c["result"], c
    with pytest.raises(NotImplementedError):
        parse_crop_borders((1, 2, 3), (97, 131))
    with pytest.raises(AssertionError):
        parse_crop_borders((0, 200, 0, 100), (97, 131))


@pytest.mark.parametrize("n_in,n_out", [(1242, 1280), (375, 384), (1226, 640), (370, 192), (131, 192), (97, 64), (70, 33), (1, 5), (7, 3), (2000, 100)])
def test_lanczos_coeffs_equal_the_restatement(n_in, n_out):
    from mindtheedge_amd.datasets.image_prep import lanczos_coeffs
    kk, bounds = lanczos_coeffs(n_in, n_out)
    want_kk, want_b = R.precompute_coeffs(n_in, n_out)
    np.testing.assert_array_equal(kk.numpy(), want_kk)
    np.testing.assert_array_equal(bounds.numpy(), want_b)
    assert kk.shape[1] == 2 * int(np.ceil(3 * max(n_in / n_out, 1.0))) + 1
    # what the kernels rely on: taps stay inside the source, both ends of the tap window never move backwards
    b = bounds.numpy().astype(np.int64)
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] >= 1).all() and (b[:, 1] <= kk.shape[1]).all()
    assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()


def test_equal_sizes_give_the_identity_table():
    from mindtheedge_amd.datasets.image_prep import lanczos_coeffs
    kk, bounds = lanczos_coeffs(64, 64)
    assert kk.shape == (64, 1) and int(kk.min()) == int(kk.max()) == 1 << 22
    np.testing.assert_array_equal(bounds.numpy(), np.stack([np.arange(64), np.ones(64)], 1))


def test_config_defaults_leave_augmentation_off():
    from mindtheedge_amd.utils.config import load_config
    cfg = load_config(None)
    assert cfg.datasets.augmentation.jittering == () and cfg.datasets.augmentation.crop_train_borders == ()
    cfg = load_config(None, {"datasets": {"augmentation": {"jittering": [0.2, 0.2, 0.2, 0.05]}}})
    assert tuple(cfg.datasets.augmentation.jittering) == (0.2, 0.2, 0.2, 0.05) and cfg.datasets.augmentation.image_shape == (384, 1280)


def test_host_tensors_are_refused():
    import torch
    from mindtheedge_amd._lib import MteError
    from mindtheedge_amd.datasets.image_prep import color_jitter_to_tensor, resize_image_u8
    with pytest.raises(MteError):
        resize_image_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), (8, 8))
    with pytest.raises(MteError):
        color_jitter_to_tensor(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


def test_compiled_kernels_do_not_pack_bytes_with_ashr_pk(tmp_path):
    """csrc/image_prep.hip::clip8 keeps its result opaque so that hipcc does not fuse the clips and the byte packing into
    v_ashr_pk_u8_i32 (on the MI355X the upper two bytes of the packed word then held stale register contents)."""
    import subprocess
    from mindtheedge_amd import _build
    out = tmp_path / "image_prep.s"
    cmd = [_build._hipcc()] + _build.FLAGS + ["-S", "--cuda-device-only", os.path.join(_build.CSRC, "image_prep.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    text = out.read_text()
    assert "resample_fused_kernel" in text and "v_ashr_pk_u8_i32" not in text
    import re
    assert all(int(m) == 0 for m in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text))
