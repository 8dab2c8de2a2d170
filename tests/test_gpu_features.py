"""rt_render_features (features.hip; include/shirley_rt.h ABI 10) against the CPU oracle: per-pixel sums of
albedo, normal and depth along each sample's own path.  The test follows the definition with the oracle's
building blocks — or_pixel_ray, or_probe_segment with the path's running draw counter, or_scene_hit_at and
or_texture_value — and compares the sums.

Normal and depth sums must be bit-identical.  The albedo passes through the marble's sin (ocml on the device,
glibc in the oracle), so it follows the project's one parity rule: >= 99 % of the channels
bit-identical and |gpu - oracle| <= 1e-10 * spp on >= 99.9 % of the pixels."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu
SEED = 0x5EED
SPP = 4
W, H = 44, 28  # 6 x 4 tiles: the last tile column holds 4 pixel columns, the last tile row 4 pixel rows


def pinhole(width, height):
    cam = rt.CameraBuilder(width=width, aspect_ratio=(width, height), vfov=20.0, focal_length=1.0).build(
        rt.CameraPosition((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), focus_length=10.0))
    assert (cam.image_width, cam.image_height, cam.has_lens) == (width, height, 0)
    return cam


def first_segment_draw(cam, seed, pixel, s):
    """The path's draw counter after the camera ray: 2 jitter draws, then two per lens-disk attempt
    (random_in_unit_disk: x, y in [-1, 1), accepted when x^2 + y^2 <= 1).  Returns (draw, attempts)."""
    if not cam.has_lens:
        return 2, 0
    draw, attempts = 2, 0
    while True:
        x = -1.0 + 2.0 * O.lib().or_rng_f64(seed, pixel, s, draw)
        y = -1.0 + 2.0 * O.lib().or_rng_f64(seed, pixel, s, draw + 1)
        draw += 2
        attempts += 1
        if x * x + y * y <= 1.0:
            return draw, attempts


def oracle_features(scene, cam, seed, s_begin, s_end, chain):
    """(albedo, normal, depth sums, most lens-disk attempts of a sample) by the definition, in sample order."""
    osc, L, d = O.OracleScene(scene), O.lib(), scene.desc
    h, w = cam.image_height, cam.image_width
    albedo, normal, depth = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
    ray, tv = O._d6(), (C.c_double * 3)()
    most = 0
    for py in range(h):
        for px in range(w):
            pixel = py * w + px
            for s in range(s_begin, s_end):
                L.or_pixel_ray(C.byref(cam), seed, px, py, s, ray)
                draw, attempts = first_segment_draw(cam, seed, pixel, s)
                most = max(most, attempts)
                r = list(ray)
                pr = osc.probe(r, seed, pixel, s, draw)
                depth[py, px] += pr.t if pr.object >= 0 else 0.0
                left = chain
                while (pr.object >= 0 and d.materials[d.objects[pr.object].material].kind == N.RT_MAT_DIELECTRIC
                       and pr.scattered and left > 0):
                    left -= 1
                    r = list(pr.origin) + list(pr.direction)
                    pr = osc.probe(r, seed, pixel, s, pr.draw)
                if pr.object < 0:
                    albedo[py, px] += list(pr.emitted)  # the sky colour of that ray; normal 0
                    continue
                m = d.materials[d.objects[pr.object].material]
                if m.kind == N.RT_MAT_METAL:
                    a = list(m.albedo)
                elif m.kind == N.RT_MAT_DIELECTRIC:
                    a = [1.0, 1.0, 1.0]
                else:
                    hit = osc.hit(r, index=pixel)
                    assert hit.hit and hit.object == pr.object and hit.t == pr.t
                    L.or_texture_value(osc.h, m.texture, hit.u, hit.v, hit.point, tv)
                    a = list(tv)
                albedo[py, px] += a
                normal[py, px] += list(pr.normal)
    return albedo, normal, depth, most


def check(got, want, spp, label):
    (ga, gn, gz), (wa, wn, wz) = got, want[:3]
    assert np.array_equal(gn, wn), f"{label}: normal sums differ on {int(np.sum(np.any(gn != wn, axis=-1)))} pixels"
    assert np.array_equal(gz, wz), f"{label}: depth sums differ on {int(np.sum(gz != wz))} pixels"
    exact = float(np.mean(ga == wa))
    close = float(np.mean(np.all(np.abs(ga - wa) <= 1e-10 * spp, axis=-1)))
    print(f"{label}: albedo channels bit-identical {exact:.4f}, pixels within 1e-10*spp {close:.4f}")
    assert exact >= 0.99 and close >= 0.999


@pytest.fixture(scope="module")
def scene():
    return rt.scenes.random_scene(SEED).finalize(SEED)


def settings(spp=SPP, **kw):
    return rt.RenderSettings(samples=spp, seed=SEED, **kw)


@pytest.mark.parametrize("chain", [0, 8])
def test_pinhole_features_match_the_oracle(gpu, scene, chain):
    cam = pinhole(W, H)
    gpu.upload(scene)
    got = gpu.render_features(cam, settings(), chain=chain)
    want = oracle_features(scene, cam, SEED, 0, SPP, chain)
    check(got, want, SPP, f"random {W}x{H} pinhole chain {chain}")
    assert np.any(got[1] != 0.0) and np.any(got[2] == 0.0)  # surfaces and sky are both in the frame
    if chain == 8:
        # the ground is a dielectric coat over the marble: first-hit features see only glass there
        first = gpu.render_features(cam, settings(), chain=0)[0]
        assert np.mean(np.all(first == SPP, axis=-1)) > 0.2 > np.mean(np.all(got[0] == SPP, axis=-1))


def test_lens_camera_features_match_the_oracle(gpu, scene):
    cam = rt.scene_camera("random", W, "std16x9")
    assert cam.has_lens and cam.image_width == W
    gpu.upload(scene)
    got = gpu.render_features(cam, settings(), chain=8)
    want = oracle_features(scene, cam, SEED, 0, SPP, 8)
    assert want[3] > 1, "no sample of the frame rejected a lens-disk point: change the seed"
    check(got, want, SPP, f"random {W}x{cam.image_height} lens chain 8")


def test_node_placements_give_identical_buffers(gpu, scene):
    cam = pinhole(W, H)
    res = []
    for nodes in ("global", "lds", "auto"):
        gpu.upload(scene, nodes=nodes)
        res.append(gpu.render_features(cam, settings(), chain=8))
    gpu.upload(scene)
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


def test_sample_ranges_add_up(gpu, scene):
    cam = pinhole(W, H)
    gpu.upload(scene)
    full = gpu.render_features(cam, settings(), chain=8)
    lo = gpu.render_features(cam, settings(sample_begin=0, sample_count=2), chain=8)
    hi = gpu.render_features(cam, settings(sample_begin=2, sample_count=2), chain=8)
    two = gpu.render_features(cam, settings(spp=2), chain=8)
    for f, a, b, t in zip(full, lo, hi, two):
        assert np.array_equal(a, t)  # the first range holds the in-order sums of samples 0, 1
        assert not np.array_equal(a, b)
        assert np.all(np.abs((a + b) - f) <= 1e-12 * np.abs(f))
    # outputs may be NULL one by one
    p = settings().params()
    depth = np.zeros((H, W))
    assert N.rt_lib().rt_render_features(gpu.handle, C.byref(cam), C.byref(p), 8, None, None,
                                         depth.ctypes.data) == N.RT_OK
    assert np.array_equal(depth, full[2])


def test_cornell_normals_and_depth_are_bit_identical(gpu):
    sc = rt.SceneBuilder.builtin("cornell", SEED).finalize(SEED)
    cam = rt.cornell_camera(40)
    gpu.upload(sc)
    got = gpu.render_features(cam, settings(), chain=0)
    want = oracle_features(sc, cam, SEED, 0, SPP, 0)
    check(got, want, SPP, "cornell 40x40 chain 0")


def test_book2_scene_is_unsupported_and_bad_arguments_are_invalid(gpu, scene):
    cam = pinhole(W, H)
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    with pytest.raises(rt.RtError) as e:
        gpu.render_features(cam, settings(), chain=0)
    assert e.value.code == N.RT_E_UNSUPPORTED
    gpu.upload(scene)
    for bad in (dict(chain=-1), dict(tile_world=2), dict(sample_begin=3, sample_count=2)):
        chain = bad.pop("chain", 0)
        with pytest.raises(rt.RtError) as e:
            gpu.render_features(cam, settings(**bad), chain=chain)
        assert e.value.code == N.RT_E_INVALID


def test_device_variant_equals_the_host_copy(gpu, scene):
    import torch
    cam = pinhole(W, H)
    gpu.upload(scene)
    host = gpu.render_features(cam, settings(), chain=8)
    a = torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda")
    n = torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda")
    z = torch.full((H, W), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_features_device(cam, settings(), 8, a.data_ptr(), n.data_ptr(), z.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for h_, d_ in zip(host, (a, n, z)):
        assert np.array_equal(h_, d_.cpu().numpy())
