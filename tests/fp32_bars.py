"""Per-pixel bars for the FP32 frames (RT_FLAG_FP32, the rtf kernels), built from
the oracle alone (DESIGN.md Numerics, "FP32 frames by stability bars").

Model.  A correct FP32 trace is the FP64 trace with every intermediate moved
by a few u = 2^-24.  How far a sample's colour may move under that is measured
on the reference itself: the frame's own 8 W H rays (oracle_frame_rays) are
traced again (oracle_trace_rays) under five probes,
    three times  (o, d + DELTA e),
    once         (o + DELTA max(1, |o|) e, d),
    once         (o, d) on scene32: every real number of the scene's JSON, and
                 of the directional lights attached to it, rounded to float32,
with DELTA = 128 u and seeded random unit vectors e.  V_s is the largest change
of any channel of a sample's colour under any probe, and
    bar(pixel) = mean over its 8 samples of (2 V_s + 16 u).
The factor 2 covers the directions three draws do not sample; 16 u is the
rounding of a colour that does not depend on the ray at all (at most 16 float
operations: an ambient product and a clamp).  A sample next to a silhouette,
a shadow edge or a total-internal-reflection switch flips under a probe: its
V_s is of order 1 and its pixel is left UNCONSTRAINED (bar > 1e-3); how many
such pixels a frame may have is a condition on the inputs, capped by
tests/test_fp32_bars.py.  Nothing here is taken from the kernels under test,
and DELTA, the factor and the floor are not tuned to a case.

Paper frames are discrete: a pixel is STABLE when four oracle paper frames
from cameras whose eye and P are each moved by DELTA max(1, |v|) e, and the
paper frame of scene32, all leave it unchanged.  On the stable pixels the FP32
paper frame must be the oracle's bit for bit.

Exceptions exist only through EXCEPTIONS below, each (case, cause, bar
multiplier) with the scene and the pixels it is for; the excepted pixels of a
case may not exceed 0.5 % of its frame.

Every reference is computed once per (scene, seed), shared, and read-only."""
import concurrent.futures
import ctypes as C
import fnmatch
import json
import zlib

import numpy as np

U = 2.0 ** -24
DELTA = 128 * U
FLOOR = 16 * U
UNCONSTRAINED = 1e-3     # a pixel whose bar exceeds this is unconstrained
N_DIR_PROBES = 3
N_PAPER_PROBES = 4
EXCEPTED_SHARE = 0.005   # of a frame's pixels, at the most, through EXCEPTIONS
THREADS = 8

# (case, cause, bar multiplier, scene, pixels).  case: the ids held32() is called with, as an fnmatch pattern
# (one scene's frame under several flags and rows is one entry); the multiplier holds at the listed (y, x)
# pixels of that scene's frame and nowhere else.  Every cause is shown on the reference alone, without a
# device, by tests/test_fp32_bars.py::test_every_exception_is_shown_on_the_reference: at each listed pixel
# DENSE_PROBES direction probes of the cause's own magnitude give a bar at least `multiplier` times the
# pixel's bar, which is to say that the pixel does sit next to a decision edge and three draws missed it.
#   named: V undersampled         probes of DELTA = 128 u, the model's own bound: V_s is a maximum over directions
#                                 and three draws found less of it than the factor 2 makes up for
EXCEPTIONS = ()   # (none was needed: the largest |d| / bar measured on an MI355X is 0.25)
DENSE_PROBES = 64
CAUSE_PROBE = {"named: V undersampled": DELTA}


def _named(case_id):
    for pattern, cause, mult, _, pixels in EXCEPTIONS:
        if fnmatch.fnmatchcase(case_id, pattern):
            return cause, float(mult), pixels
    return None, 1.0, ()


assert all(cause in CAUSE_PROBE and mult > 1.0 and pixels for _, cause, mult, _, pixels in EXCEPTIONS)


def seed_of(name: str) -> int:
    """The probes' seed for a scene name (one np.random.default_rng seed each)."""
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------- scene32
def _round32(v):
    if isinstance(v, float):
        with np.errstate(over="ignore"):
            return float(np.float32(v))
    if isinstance(v, int) and not isinstance(v, bool):
        assert abs(v) <= 2 ** 24, v   # (exact in float32: stays the integer the schema may require)
        return v
    if isinstance(v, list):
        return [_round32(x) for x in v]
    if isinstance(v, dict):
        return {k: _round32(x) for k, x in v.items()}
    return v


def scene32(text, dir_lights=None):
    """(text, dir_lights) with every real number rounded to float32 and back."""
    lights = None if dir_lights is None else [tuple([float(np.float32(x)) for x in v] for v in l) for l in dir_lights]
    return json.dumps(_round32(json.loads(text))), lights


def load(rt, text, dir_lights=None):
    sc = rt.load_scene_from_json_text(text)
    return rt.with_dir_lights(sc, dir_lights) if dir_lights else sc


# --------------------------------------------------------------------- trace
def trace(rt, sc, o, d):
    """oracle_trace_rays of (n, 3) rays on THREADS threads (the call keeps no
    state between rays and releases the interpreter): (rgb, n_intersect, n_occluded)."""
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    rt.oracle_trace_rays(sc, o[:1], d[:1])   # (the library is loaded and its prototype set before the threads start)
    cuts = np.linspace(0, len(o), THREADS + 1).astype(int)
    with concurrent.futures.ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda k: rt.oracle_trace_rays(sc, o[cuts[k]:cuts[k + 1]], d[cuts[k]:cuts[k + 1]]),
                            range(THREADS)))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def unit_vectors(rng, n):
    e = rng.normal(size=(n, 3))
    return e / np.sqrt((e * e).sum(axis=1))[:, None]


def resolve(rgb, H, W):
    """The frame of (H W 8, 3) sample colours as tracer.cpp sums them: in order, then times 1/8."""
    c = rgb.reshape(H, W, 8, 3)
    acc = np.zeros((H, W, 3))
    for s in range(8):
        acc = acc + c[:, :, s]
    return acc * (1.0 / 8)


class Standard:
    """A standard frame's references: rays o, d (H W 8, 3), their colours rgb,
    ref (H, W, 3), V (H, W, 8), bar (H, W), unconstrained (H, W), counts."""


_standard, _paper = {}, {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def standard_case(rt, text, dir_lights=None, seed=0) -> Standard:
    key = (text, repr(dir_lights), seed)
    if key in _standard:
        return _standard[key]
    sc = load(rt, text, dir_lights)
    text32, lights32 = scene32(text, dir_lights)
    sc32 = load(rt, text32, lights32)
    W, H = sc.width, sc.height
    assert (sc32.width, sc32.height) == (W, H)
    o, d = (v.reshape(-1, 3) for v in rt.oracle_frame_rays(sc))
    rgb, ni, no = trace(rt, sc, o, d)
    rng = np.random.default_rng(seed)
    V = np.zeros(len(o))
    for _ in range(N_DIR_PROBES):
        V = np.maximum(V, np.abs(trace(rt, sc, o, d + DELTA * unit_vectors(rng, len(o)))[0] - rgb).max(axis=1))
    size = np.maximum(1.0, np.sqrt((o * o).sum(axis=1)))[:, None]
    V = np.maximum(V, np.abs(trace(rt, sc, o + DELTA * size * unit_vectors(rng, len(o)), d)[0] - rgb).max(axis=1))
    ray_free = bool((V == 0).all())
    V = np.maximum(V, np.abs(trace(rt, sc32, o, d)[0] - rgb).max(axis=1))
    assert np.isfinite(V).all() and np.isfinite(rgb).all()
    r = Standard()
    r.W, r.H, r.o, r.d, r.rgb = W, H, o, d, rgb
    r.ref = resolve(rgb, H, W)
    r.V = V.reshape(H, W, 8)
    r.bar = (2.0 * r.V + FLOOR).mean(axis=2)
    r.unconstrained = r.bar > UNCONSTRAINED
    r.counts = (int(ni.sum()), int(no.sum()))
    # no sample's colour moves with its ray (under the four ray probes; scene32 may still move the one colour
    # such a frame has by its own rounding, 8e-10 on inside_camera): no decision of the trace is near its
    # edge, so the ray counts are held to the oracle's too
    r.ray_free = ray_free
    _frozen(r.o, r.d, r.rgb, r.ref, r.V, r.bar, r.unconstrained)
    _standard[key] = r
    return r


def standard_bars(rt, text, dir_lights=None, seed=0):
    """(ref, bar, unconstrained mask) of the standard frame of a scene."""
    r = standard_case(rt, text, dir_lights, seed)
    return r.ref, r.bar, r.unconstrained


def _moved_camera(rt, sc, rng):
    d = rt.SceneDesc.from_buffer_copy(sc.desc)
    for field in (d.camera.eye, d.camera.P):
        v = np.array(list(field))
        v = v + DELTA * max(1.0, float(np.sqrt((v * v).sum()))) * unit_vectors(rng, 1)[0]
        field[:] = v.tolist()
    return rt.scene_from_desc(d)


def paper_stable(rt, text, dir_lights=None, seed=0):
    """(ref, stable mask) of the paper frame of a scene."""
    key = (text, repr(dir_lights), seed)
    if key in _paper:
        return _paper[key]
    sc = load(rt, text, dir_lights)
    W, H = sc.width, sc.height
    ref, _ = rt.oracle_render(sc, W, H, 1, threads=THREADS)
    rng = np.random.default_rng(seed)
    stable = np.ones((H, W), dtype=bool)
    others = [_moved_camera(rt, sc, rng) for _ in range(N_PAPER_PROBES)] + [load(rt, *scene32(text, dir_lights))]
    for other in others:
        assert (other.width, other.height) == (W, H)
        fb, _ = rt.oracle_render(other, W, H, 1, threads=THREADS)
        stable &= (fb == ref).all(axis=2)
    _frozen(ref, stable)
    _paper[key] = (ref, stable)
    return _paper[key]


# ---------------------------------------------------------------------- held
def held32(case_id, fb, ref, bar):
    """fb against ref (H, W, 3) under bar (H, W): every channel of every pixel
    within its pixel's bar, but for EXCEPTIONS; prints the case's line and
    returns the largest |d| / bar."""
    fb = np.ascontiguousarray(fb, dtype=np.float64)
    assert fb.shape == ref.shape and bar.shape == ref.shape[:2], (case_id, fb.shape, ref.shape, bar.shape)
    assert (bar >= FLOOR).all(), case_id
    n = bar.size
    with np.errstate(invalid="ignore"):
        ratio = np.nan_to_num(np.abs(fb - ref).max(axis=2) / bar, nan=np.inf)   # (a NaN channel is over every bar)
    cause, mult, pixels = _named(case_id)
    allowed = np.ones(bar.shape)
    for y, x in pixels:
        allowed[y, x] = mult
    over = ratio > 1.0
    wrong = ratio > allowed
    excepted = int(over.sum()) - int(wrong.sum())
    line = (f"  {case_id}: {n} pixels, {float(np.mean(bar > UNCONSTRAINED)):.4%} unconstrained, {int(wrong.sum())} over the bar, "
            f"|d|/bar largest {float(ratio.max()):.3g} median {float(np.median(ratio)):.3g}")
    if cause is not None:
        line += f"; {cause}: {excepted} of the {len(pixels)} listed pixels over the bar, within {mult:g} bars"
    print(line)
    where = [(int(y), int(x), float(ratio[y, x]), float(bar[y, x])) for y, x in np.argwhere(wrong)[:6]]
    assert not wrong.any(), (case_id, f"{int(wrong.sum())} of {n} pixels over the bar, largest ratio {float(ratio.max()):.3g}",
                             where)
    assert excepted <= EXCEPTED_SHARE * n, (case_id, f"{excepted} of {n} pixels excepted")
    return float(ratio.max())


def held32_paper(case_id, fb, ref, stable):
    """A paper frame against the oracle's, bit for bit on the stable pixels."""
    fb = np.ascontiguousarray(fb, dtype=np.float64)
    assert fb.shape == ref.shape and stable.shape == ref.shape[:2], (case_id, fb.shape, ref.shape)
    differ = (fb.view(np.uint64) != np.ascontiguousarray(ref).view(np.uint64)).any(axis=2)
    wrong = differ & stable
    print(f"  {case_id}: {stable.size} pixels, {float(np.mean(~stable)):.4%} unstable, {int(wrong.sum())} stable pixels differ, "
          f"{int((differ & ~stable).sum())} unstable ones")
    assert not wrong.any(), (case_id, f"{int(wrong.sum())} stable pixels differ", np.argwhere(wrong)[:6].tolist())
    return int(differ.sum())


# ---------------------------------------------------------- the older bars
def old_bars_pass(fb, ref, counts, ref_counts, far_frac=0.01, mean_tol=5e-3):
    """The whole-frame bars of tests/test_gpu_fp32.py, as a predicate."""
    d = np.abs(fb - ref)
    return bool(np.isfinite(fb).all() and float(np.mean(d > 1e-3)) <= far_frac and d.mean() <= mean_tol
                and abs(sum(counts) - sum(ref_counts)) <= 0.05 * sum(ref_counts) + 16)


def copy_desc(rt, sc, materials=None, lights=None):
    """Copy of a scene with every material / point light passed through a function (test mistakes)."""
    d = rt.SceneDesc.from_buffer_copy(sc.desc)
    keep = []
    if materials is not None:
        mats = (rt.Material * max(1, d.n_materials))()
        C.memmove(mats, d.materials, C.sizeof(rt.Material) * d.n_materials)
        for i in range(d.n_materials):
            materials(mats[i])
        d.materials = C.cast(mats, C.POINTER(rt.Material))
        keep.append(mats)
    if lights is not None:
        arr = (rt.Light * max(1, d.n_lights))()
        C.memmove(arr, d.lights, C.sizeof(rt.Light) * d.n_lights)
        for i in range(d.n_lights):
            lights(arr[i])
        d.lights = C.cast(arr, C.POINTER(rt.Light))
        keep.append(arr)
    return rt.scene_from_desc(d)
