"""rt_scene_occluded (occlusion.hip / occlusion.h; include/shirley_rt.h ABI 11) ray by ray against the CPU
oracle and against the closest-hit path: out[i] = 1 exactly when the oracle reports a hit on [t_min, tmax_i]
and exactly when rt_scene_hit_ex(RT_TRAVERSAL_RENDER) reports an object.  Every comparison is exact equality
over the whole batch; each batch must hold at least 15 % of either class, so that neither answer is trivial."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import raytracer as rt
from raytracer import _native as N

pytestmark = pytest.mark.gpu

SEED = 0x5EED
INF = float("inf")
PLACEMENTS = ["auto", "global", "half-lds"]


@pytest.fixture(scope="module")
def random_scene():
    scene = rt.scenes.random_scene(SEED).finalize(SEED)
    return scene, O.OracleScene(scene)


def random_batch():
    """The 4096 rays of test_render_traversal_matches_oracle, then a per-ray bound drawn next."""
    rng = np.random.default_rng(1)
    n = 4096
    orig = np.column_stack([rng.uniform(-12, 12, n), rng.uniform(0.05, 3, n), rng.uniform(-12, 12, n)])
    rays = np.hstack([orig, rng.normal(size=(n, 3))])
    t_each = np.exp(rng.uniform(np.log(0.05), np.log(20.0), n))
    return rays, t_each


def oracle_occluded(osc, rays, t_max):
    t = np.broadcast_to(np.asarray(t_max, dtype=np.float64), (len(rays),))
    return np.array([1 if osc.hit(rays[i], 0.001, float(t[i])).hit else 0 for i in range(len(rays))], dtype=np.uint8)


def both_classes(out, label):
    frac = float(np.mean(out))
    print(f"{label}: {int(out.sum())} of {len(out)} occluded")
    assert 0.15 <= frac <= 0.85, f"{label}: a class holds less than 15 % of the batch ({frac:.3f} occluded)"


@pytest.fixture(scope="module")
def random_reference(random_scene):
    """The oracle's answers on the random batch, computed once: (rays, t_each, at inf, at the per-ray bound)."""
    _, osc = random_scene
    rays, t_each = random_batch()
    return rays, t_each, oracle_occluded(osc, rays, INF), oracle_occluded(osc, rays, t_each)


@pytest.mark.parametrize("bvh", ["reference", "sah"])
@pytest.mark.parametrize("nodes", PLACEMENTS)
def test_random_scene_matches_oracle_and_closest_hit(gpu, random_scene, random_reference, nodes, bvh):
    scene, _ = random_scene
    rays, t_each, want_inf, want_each = random_reference
    gpu.upload(scene, bvh, nodes)
    got_inf = gpu.occluded(rays, 0.001, INF)
    got_each = gpu.occluded(rays, 0.001, t_each)
    assert got_inf.dtype == np.uint8 and set(np.unique(got_inf)) <= {0, 1}
    both_classes(want_inf, f"random {bvh}/{nodes} t_max inf")
    both_classes(want_each, f"random {bvh}/{nodes} per-ray t_max")
    assert np.array_equal(got_inf, want_inf)
    assert np.array_equal(got_each, want_each)
    assert int(np.sum(want_inf != want_each)) > 0  # hits beyond a ray's own bound: the bound matters
    hits = gpu.hit(rays, 0.001, INF, traversal="render")
    assert np.array_equal(got_inf, np.array([1 if h.object >= 0 else 0 for h in hits], dtype=np.uint8))


@pytest.mark.parametrize("nodes", PLACEMENTS)
def test_far_origins_take_the_f64_key_branch(gpu, random_scene, nodes):
    """The generator of test_render_traversal_far_origins (origins beyond origin_limit: node4_keys' f64 branch)
    with the direction scale kept: the target lies at t = 1 / sc, the bound at (1 / sc) U(0.5, 1.5)."""
    scene, osc = random_scene
    gpu.upload(scene, "sah", nodes)
    lim = gpu.stats().origin_limit
    assert lim >= 16.0
    rng = np.random.default_rng(3)
    n = 2048
    target = np.column_stack([rng.uniform(-11, 11, n), rng.uniform(0.0, 1.5, n), rng.uniform(-11, 11, n)])
    u = rng.normal(size=(n, 3))
    u[:, 1] = np.abs(u[:, 1])
    u /= np.linalg.norm(u, axis=1)[:, None]
    dist = lim * np.exp(rng.uniform(np.log(1.5), np.log(1000.0), n))
    orig = target + u * dist[:, None]
    assert (np.abs(orig).max(axis=1) > lim).all()
    sc = rng.uniform(0.5, 2.0, n)
    rays = np.hstack([orig, (target - orig) * sc[:, None]])
    t_each = (1.0 / sc) * rng.uniform(0.5, 1.5, n)
    want = oracle_occluded(osc, rays, t_each)
    both_classes(want, f"far origins {nodes} (limit {lim:g})")
    assert np.array_equal(gpu.occluded(rays, 0.001, t_each), want)


def rect_batch(name):
    rng = np.random.default_rng(5)
    n = 2048
    if name == "cornell":
        orig = rng.uniform(1, 554, (n, 3))
        d = rng.normal(size=(n, 3))
        t_each = np.exp(rng.uniform(np.log(1.0), np.log(1000.0), n))
    else:
        orig = np.column_stack([rng.uniform(-6, 6, n), rng.uniform(0.05, 5, n), rng.uniform(-6, 6, n)])
        d = rng.normal(size=(n, 3))
        t_each = np.exp(rng.uniform(np.log(0.05), np.log(20.0), n))
    return np.hstack([orig, d]), t_each


@pytest.mark.parametrize("nodes", PLACEMENTS)
@pytest.mark.parametrize("name", ["cornell", "box-light"])
def test_rect_and_rectbox_scenes(gpu, name, nodes):
    """Rect and RectBox leaves (the second and third leaf loops) in every node placement."""
    scene = rt.SceneBuilder.builtin(name, SEED).finalize(SEED)
    gpu.upload(scene, nodes=nodes)
    rays, t_each = rect_batch(name)
    want = oracle_occluded(O.OracleScene(scene), rays, t_each)
    both_classes(want, f"{name} {nodes}")
    assert np.array_equal(gpu.occluded(rays, 0.001, t_each), want)


@pytest.mark.parametrize("nodes", PLACEMENTS)
def test_closest_hit_instance_gives_the_same_bytes(gpu, random_scene, random_reference, monkeypatch, nodes):
    scene, _ = random_scene
    rays, t_each, want_inf, want_each = random_reference
    gpu.upload(scene, "reference", nodes)
    any_inf, any_each = gpu.occluded(rays, 0.001, INF), gpu.occluded(rays, 0.001, t_each)
    monkeypatch.setenv("SHIRLEY_OCCLUDED_CLOSEST", "1")  # read at the call
    cl_inf, cl_each = gpu.occluded(rays, 0.001, INF), gpu.occluded(rays, 0.001, t_each)
    monkeypatch.delenv("SHIRLEY_OCCLUDED_CLOSEST")
    assert any_inf.tobytes() == cl_inf.tobytes() and any_each.tobytes() == cl_each.tobytes()
    assert np.array_equal(cl_inf, want_inf) and np.array_equal(cl_each, want_each)


def test_device_form_equals_the_host_form(gpu, random_scene, random_reference):
    import torch
    scene, _ = random_scene
    rays, t_each, _, _ = random_reference
    gpu.upload(scene)
    host_inf, host_each = gpu.occluded(rays, 0.001, INF), gpu.occluded(rays, 0.001, t_each)
    r = torch.from_numpy(rays).cuda()
    t = torch.from_numpy(t_each).cuda()
    out = torch.full((len(rays),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    gpu.occluded_device(r.data_ptr(), len(rays), out.data_ptr(), 0.001, INF, 0, stream)  # t_max_each = NULL
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host_inf)
    out.fill_(7)
    gpu.occluded_device(r.data_ptr(), len(rays), out.data_ptr(), 0.001, 0.0, t.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host_each)


def test_errors(gpu, random_scene):
    scene, _ = random_scene
    lib = N.rt_lib()
    rays = np.zeros((2, 6))
    rays[:, 5] = -1.0
    out = np.zeros(2, dtype=np.uint8)
    args = (rays.ctypes.data, 2, 0.001, INF, None, out.ctypes.data)
    fresh = rt.Device(0)
    assert lib.rt_scene_occluded(fresh.handle, *args) == N.RT_E_INVALID  # no scene uploaded
    fresh.close()
    gpu.upload(rt.scenes.final_scene(SEED, 4, 30).finalize(SEED))
    assert lib.rt_scene_occluded(gpu.handle, *args) == N.RT_E_UNSUPPORTED
    with pytest.raises(rt.RtError) as e:
        gpu.occluded(rays)
    assert e.value.code == N.RT_E_UNSUPPORTED
    gpu.upload(scene)
    assert lib.rt_scene_occluded(gpu.handle, *args) == N.RT_OK
    assert lib.rt_scene_occluded(gpu.handle, None, 2, 0.001, INF, None, out.ctypes.data) == N.RT_E_INVALID
    assert lib.rt_scene_occluded(gpu.handle, rays.ctypes.data, 2, 0.001, INF, None, None) == N.RT_E_INVALID
    assert lib.rt_scene_occluded(gpu.handle, rays.ctypes.data, -1, 0.001, INF, None, out.ctypes.data) == N.RT_E_INVALID
    nan = float("nan")
    assert lib.rt_scene_occluded(gpu.handle, rays.ctypes.data, 2, nan, INF, None, out.ctypes.data) == N.RT_E_INVALID
    assert lib.rt_scene_occluded(gpu.handle, rays.ctypes.data, 2, 0.001, nan, None, out.ctypes.data) == N.RT_E_INVALID
    assert lib.rt_scene_occluded_device(gpu.handle, None, 2, 0.001, INF, None, C.c_void_p(8), None) == N.RT_E_INVALID
    assert lib.rt_scene_occluded_device(gpu.handle, C.c_void_p(8), 2, nan, INF, None, C.c_void_p(8), None) == N.RT_E_INVALID
    # an empty batch is fine
    assert lib.rt_scene_occluded(gpu.handle, rays.ctypes.data, 0, 0.001, INF, None, out.ctypes.data) == N.RT_OK
    assert len(gpu.occluded(np.zeros((0, 6)))) == 0
