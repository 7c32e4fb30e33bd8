"""GPU: the specular skip of shade()'s point-light pass 2 (rt_device.hpp
spec_skips, RT_SPEC_SKIP) in the trace kernels, bit for bit against the oracle.

A lane whose reflection vector faces away from the eye keeps Es = +0 instead
of normalising the vector and raising a zero to the shininess.  What can go
wrong is a lane that skips and should not (a shininess of 0, whose power is 1;
a product inside the margin), a wave whose lanes disagree, or a lane that
rides along inactive.  So single waves are traced: 64-ray batches of
rt_query_radiance (and one of 37 rays, and frames whose edges cut the 2x4-pixel
tiles) chosen so that every lit lane skips, none does, lanes are mixed, the
product straddles the margin, one lane has a shininess of 0 or 12.5 among
skipping lanes, and materials differ between lanes.  Which lanes skip is asked
of the device itself (rt_test_spec_skip: the predicate shade() calls, on the
oracle's hit of each ray), so a batch that is meant to skip is known to.

Bar: every colour channel bit-equal to the oracle in mode 1 (rtamd.oracle_pow:
libm everywhere but pow_spec's correctly rounded integer powers), and the
Scene::occluded counts equal.  Rays that hit the 12.5 sphere with the power
actually evaluated are not drawn: that power is the device library's, held to
libm in ulps by tests/test_gpu_rounding.py; the one such lane used here has
r.v = 0, where both libraries return 0."""
import functools
import json
import math

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

FRONT = ([0.3, 1.8, 4.0], [3.0, 2.5, 2.0])    # on the eye's side: the floor's reflections run away from the eye
BACK = ([-0.5, 3.0, -7.0], [4.0, 4.0, 5.0])   # beyond the objects: the floor's reflections run towards the eye
EYE = np.array([0.0, 0.3, 5.0])
MARGIN = 2.0 ** -40


def _mat(col, shin, spec=0.4):
    return {"diffuse": col, "ambient": [0.05, 0.05, 0.05], "specular": [spec, spec, spec], "shininess": shin}


def _sph(p, r, m):
    return {"sphere": {"position": p, "radius": r, "color": m}}


def _scene_dict():
    objs = [
        {"halfSpace": {"position": [0, -1.2, 0], "normal": [0, 1, 0], "color": _mat([0.5, 0.6, 0.5], 24)}},
        _sph([-1.3, -0.5, -1.0], 0.7, _mat([0.8, 0.3, 0.2], 32)),
        _sph([0.9, -0.4, -1.6], 0.8, _mat([0.2, 0.5, 0.8], 12)),
        _sph([-0.2, 0.7, -2.6], 0.6, _mat([0.3, 0.8, 0.3], 1)),
        _sph([1.7, 0.7, -0.8], 0.4, _mat([0.8, 0.8, 0.2], 0)),       # pow(x, 0) = 1: never skipped
        _sph([-1.7, 0.9, -1.8], 0.45, _mat([0.7, 0.3, 0.7], 12.5)),  # the library's pow: never skipped
    ]
    return {
        "screen": {"dpi": 8, "dimensions": [4, 3], "position": [-2, -1.5, 0], "observer": EYE.tolist()},
        "medium": {"ambient": [0.2, 0.2, 0.2], "index": 1.0, "recursion": 1},
        "background": [0.3, 0.4, 0.6],
        "sources": [{"position": p, "intensity": i} for p, i in (FRONT, BACK)],
        "objects": objs,
    }


@functools.lru_cache(maxsize=None)
def _scenes(rt):
    both = rt.load_scene_from_json_text(json.dumps(_scene_dict()))
    return {"both": both, "front": rt.with_point_lights(both, [FRONT]), "back": rt.with_point_lights(both, [BACK])}


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _normalized(v):
    L = np.sqrt(_dot(v, v))
    with np.errstate(all="ignore"):
        return np.where((L > 1e-6)[:, None], v / L[:, None], np.array([0.0, 1.0, 0.0]))


class Lanes:
    """Per (ray, light) of a scene, from the oracle's hit of each ray, in
    shade()'s own operations: lit (the light reaches pass 2), skip (the
    device's predicate, rt_test_spec_skip), would (the predicate at a shininess
    of 24 instead of the material's), u = dot3(rv, wo), plain (the power the
    device computes without the skip); mat, shin, ks per ray."""

    def __init__(self, rt, sc, o, d):
        dsc = sc.desc
        n = len(o)
        ok, hits = rt.oracle_scene_intersect(sc, rt.make_rays(o, d))
        self.mat = np.where(ok, hits["mat"], -1)
        m = np.clip(self.mat, 0, None)
        self.shin = np.array([dsc.materials[i].shininess for i in range(dsc.n_materials)])[m]
        self.ks = np.array([dsc.materials[i].ks for i in range(dsc.n_materials)])[m]
        p, nn, t = hits["p"], hits["n"], hits["t"]
        wo = _normalized(-_normalized(np.asarray(d, dtype=np.float64)))
        eps = np.where(1e-3 < 1e-4 * t, 1e-4 * t, 1e-3)
        so = p + nn * eps[:, None]
        nl = dsc.n_lights
        self.lit, self.skip, self.would = (np.zeros((n, nl), dtype=bool) for _ in range(3))
        self.u, self.plain = np.zeros((n, nl)), np.zeros((n, nl))
        for li in range(nl):
            tl = np.array(list(dsc.lights[li].pos)) - p
            d2 = _dot(tl, tl)
            d2 = np.where(d2 <= 0.01, 0.01, d2)
            dist = np.sqrt(d2)
            wi = tl / dist[:, None]
            max_t = dist - eps
            need = ok & (_dot(nn, wi) > 0.0) & (max_t > eps)
            k = np.flatnonzero(need)
            lit = np.zeros(n, dtype=bool)
            lit[k] = ~rt.oracle_occluded(sc, so[k], wi[k], eps[k], max_t[k])
            self.lit[:, li] = lit
            ndw = _dot(nn, wi)
            rv = (2.0 * ndw)[:, None] * nn - wi
            self.u[:, li] = _dot(rv, wo)
            spec = lit & (self.ks > 0.0)
            sk, pl = rt.spec_skip(nn, wi, wo, self.shin)
            self.skip[:, li], self.plain[:, li] = sk & spec, pl
            self.would[:, li] = rt.spec_skip(nn, wi, wo, np.full(n, 24.0))[0] & spec
        # the device's own arithmetic agrees: wherever it skips, the power it would have computed is +-0
        assert np.all(self.plain[self.skip] == 0.0)
        self.n_spec = (self.lit & (self.ks > 0.0)[:, None]).sum(axis=1)


def _eye_rays(n, seed):
    """Rays from the eye through random points of the screen rectangle."""
    rng = np.random.default_rng(seed)
    tgt = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), np.zeros(n)], axis=1)
    o = np.tile(EYE, (n, 1))
    return o, tgt - o


@functools.lru_cache(maxsize=None)
def _pool(rt, which):
    """1536 eye rays of scene `which` and their lanes, classified once."""
    o, d = _eye_rays(1536, 11)
    return o, d, Lanes(rt, _scenes(rt)[which], o, d)


def _check(rt, sc, o, d, what):
    """The batch as one radiance query against the mode-1 oracle: every channel's bits, the occlusion counts."""
    st = rt.Stats()
    got = rt.query_radiance(sc, o, d, 0, st)
    with rt.oracle_pow(rt.ORACLE_POW_DEVICE):
        ref, ni, no = rt.oracle_trace_rays(sc, o, d)
    diff = np.flatnonzero((got.view(np.uint64) != ref.view(np.uint64)).any(axis=1))
    print(f"  {what}: {len(o)} rays, {len(diff)} differ, occluded calls {int(st.rays_occluded)} (oracle {int(no.sum())})")
    assert len(diff) == 0, (what, diff[:8], [(got[k], ref[k]) for k in diff[:3]])
    assert (int(st.rays_intersect), int(st.rays_occluded)) == (int(ni.sum()), int(no.sum())), what


def _pick(mask, n, what):
    k = np.flatnonzero(mask)
    assert len(k) >= n, (what, len(k))
    return k[:n]


NOT_LIB = lambda ln: ln.shin != 12.5   # noqa: E731  (no lane whose power is the library's)


def test_every_lit_lane_skips(gpu):
    """(a) One light on the eye's side; 64 lanes, each with a specular term to leave out, none to compute."""
    o, d, ln = _pool(gpu, "front")
    k = _pick((ln.n_spec > 0) & (ln.skip.sum(axis=1) == ln.n_spec), 64, "all skip")
    assert ln.skip[k].all() and ln.lit[k].all()
    _check(gpu, _scenes(gpu)["front"], o[k], d[k], "every lit lane skips")


def test_no_lane_skips(gpu):
    """(b) One light beyond the objects; 64 lit lanes with a specular term, none skipping."""
    o, d, ln = _pool(gpu, "back")
    k = _pick((ln.n_spec > 0) & ~ln.skip.any(axis=1) & NOT_LIB(ln), 64, "none skips")
    _check(gpu, _scenes(gpu)["back"], o[k], d[k], "no lane skips")


def test_mixed_lanes_and_materials(gpu):
    """(c), (h) Both lights: in each light's iteration some lanes skip and some
    do not, over at least four materials; lanes that miss and lanes in shadow
    ride along."""
    o, d, ln = _pool(gpu, "both")
    k = _pick(NOT_LIB(ln), 64, "mixed")
    spec = ln.lit[k] & (ln.ks[k] > 0.0)[:, None]
    for li in range(2):
        assert ln.skip[k, li].any() and (spec[:, li] & ~ln.skip[k, li]).any(), li
    assert len(set(ln.mat[k].tolist()) - {-1}) >= 4
    _check(gpu, _scenes(gpu)["both"], o[k], d[k], "mixed lanes")
    # the same rays, the two kinds interleaved lane by lane (alternating all-skip and no-skip floor hits)
    a = _pick(ln.skip[:, 0] & ~ln.skip[:, 1] & (ln.n_spec == 2), 32, "skip under the front light only")
    b = _pick(~ln.skip.any(axis=1) & (ln.n_spec > 0) & NOT_LIB(ln), 32, "no skip")
    k2 = np.stack([a, b], axis=1).reshape(-1)
    _check(gpu, _scenes(gpu)["both"], o[k2], d[k2], "interleaved lanes")


def _margin_rays(rt):
    """64 rays onto one floor point under the front light, the eye swung in
    the light's plane so that u = dot3(rv, wo) runs through 0 in steps of about
    2^-43: the margin -2^-40 lies inside the batch."""
    sc = _scenes(rt)["front"]
    p0 = np.array([0.3, -1.2, 1.0])

    def rays(th):
        th = np.atleast_1d(th)
        o = p0 + 4.0 * np.stack([np.zeros_like(th), np.sin(th), np.cos(th)], axis=1)
        return o, p0 - o

    lo, hi = 0.6, 1.0   # u = -cos(light's elevation + eye's elevation): the light stands at 45 degrees
    f = lambda th: Lanes(rt, sc, *rays(th)).u[0, 0]   # noqa: E731
    assert f(lo) < 0.0 < f(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if f(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    th = lo + 2.0 ** -43 * np.arange(-40, 24)
    return sc, rays(th)


def test_margin_is_straddled(gpu):
    """(d) u on both sides of the margin and of zero in one wave: lanes below
    -2^-40 skip, lanes between -2^-40 and 0 and lanes above 0 do not."""
    sc, (o, d) = _margin_rays(gpu)
    ln = Lanes(gpu, sc, o, d)
    u = ln.u[:, 0]
    assert ln.lit[:, 0].all() and np.abs(u).max() < 2.0 ** -36
    assert np.array_equal(ln.skip[:, 0], u <= -MARGIN)
    inside = (u > -MARGIN) & (u < 0.0)
    print(f"  margin: {int(ln.skip[:, 0].sum())} lanes skip, {int(inside.sum())} inside the margin, {int((u > 0).sum())} above 0")
    assert ln.skip[:, 0].sum() >= 8 and inside.sum() >= 4 and (u > 0.0).sum() >= 8
    _check(gpu, sc, o, d, "margin")


@pytest.mark.parametrize("shin", [0.0, 12.5])
def test_one_lane_keeps_its_term_among_skipping_lanes(gpu, shin):
    """(e), (f) 63 skipping lanes and one whose reflection faces away as well
    but whose shininess is 0 (the power is 1, the term is not 0) or 12.5 (the
    library's pow, of a zero): it takes today's path."""
    o, d, ln = _pool(gpu, "front")
    k = _pick((ln.n_spec > 0) & (ln.skip.sum(axis=1) == ln.n_spec), 63, "all skip")
    odd = _pick((ln.shin == shin) & ln.would[:, 0] & ~ln.skip[:, 0], 1, f"a lane of shininess {shin}")
    assert ln.plain[odd[0], 0] == (1.0 if shin == 0.0 else 0.0)
    k = np.insert(k, 29, odd[0])
    _check(gpu, _scenes(gpu)["front"], o[k], d[k], f"one lane of shininess {shin}")


def test_partial_wave(gpu):
    """(g) 37 rays: a wave with 27 lanes off."""
    o, d, ln = _pool(gpu, "both")
    k = _pick(NOT_LIB(ln), 37, "partial")
    assert ln.skip[k].any()
    _check(gpu, _scenes(gpu)["both"], o[k], d[k], "37 rays")


# ------------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def _cfg4(rt):
    """The benchmark's scene at 13x7: the frame's edges cut the 2x4-pixel tiles."""
    return rt.load_scene_from_json_text(json.dumps(scenes.with_size(scenes.cfg4_scene(), 13, 7, 3)))


def test_bench_kernel_frame_and_op_counts(gpu):
    """The benchmark's kernel and its op-counting builds on a frame with
    partial waves: the frame bit-equal to the mode-1 oracle's, and shade_spec
    (with shade_light and shade_call) the oracle's count while lanes skip: the
    counter counts the reference's calls, skipped or not."""
    rt = gpu
    sc = _cfg4(rt)
    assert rt.kernel_name(sc, 0) == (0, "rtd::k_std_lean<false, 1, false>")
    o, d = rt.oracle_frame_rays(sc)
    ln = Lanes(rt, sc, o.reshape(-1, 3), d.reshape(-1, 3))
    n_skip, n_spec = int(ln.skip.sum()), int(ln.n_spec.sum())
    print(f"  13x7 frame: {n_skip} of {n_spec} specular terms skipped")
    assert n_skip > 0 and n_skip < n_spec
    with rt.oracle_pow(rt.ORACLE_POW_DEVICE):
        ref, ost = rt.oracle_render(sc, 13, 7, 0, threads=8)
    want = {nm: int(ost.ops[i]) for i, nm in enumerate(rt.OP_NAMES)}
    assert want["shade_spec"] == n_spec
    for flags in (0, rt.RT_FLAG_COUNT_OPS, rt.RT_FLAG_COUNT_OPS | rt.RT_FLAG_NO_CULL):
        st = rt.Stats()
        fb = rt.Tracer(sc, 13, 7, 0, flags=flags).render(st)
        assert np.array_equal(fb.view(np.uint64), ref.view(np.uint64)), flags
        assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
        if flags:
            got = {nm: int(st.ops[i]) for i, nm in enumerate(rt.OP_NAMES)}
            for nm in ("shade_spec", "shade_light", "shade_call"):
                assert got[nm] == want[nm], (flags, nm, got[nm], want[nm])


def test_own_scene_frame(gpu):
    """The test scene as a 32x24 frame (jittered rays, recursion off), both lights."""
    rt = gpu
    sc = _scenes(rt)["both"]
    assert (sc.width, sc.height) == (32, 24)
    st = rt.Stats()
    fb = rt.Tracer(sc, 32, 24, 0).render(st)
    with rt.oracle_pow(rt.ORACLE_POW_DEVICE):
        ref, ost = rt.oracle_render(sc, 32, 24, 0, threads=8)
    lib = np.zeros((24, 32), dtype=bool)   # pixels with a sample on the 12.5 sphere: the library's pow, not compared
    o, d = rt.oracle_frame_rays(sc)
    ln = Lanes(rt, sc, o.reshape(-1, 3), d.reshape(-1, 3))
    lib |= (ln.shin == 12.5).reshape(24, 32, 8).any(axis=2)
    assert ln.skip.any() and lib.sum() < 40
    same = (fb.view(np.uint64) == ref.view(np.uint64)).all(axis=2)
    assert same[~lib].all(), np.argwhere(~same & ~lib)[:8]
    assert (st.rays_intersect, st.rays_occluded) == (ost.rays_intersect, ost.rays_occluded)
    assert math.isfinite(float(fb.sum()))
