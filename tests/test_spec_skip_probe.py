"""CPU: the specular skip's exactness probe (tools/probe/spec_skip_check.c).

shade()'s point-light pass 2 leaves the specular term out of lanes whose
reflection faces away from the eye (rt_device.hpp spec_skips, RT_SPEC_SKIP).
The probe evaluates one lit (sample, light) both ways in host double
arithmetic, without FMA contraction, and fails on any case where the skip
condition holds and the colour is not bit-equal, the clamped r.v is not +-0,
or a guard (shininess <= 0, a NaN, normalized()'s fallback) was passed.  The
full run is 50 M cases; here a reduced count, the same
case mix, in about a second."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "probe", "spec_skip_check.c")
CASES = 2_000_000


def test_spec_skip_probe(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "spec_skip_check")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-Wall", "-Werror", SRC, "-lm", "-o", exe], check=True)
    r = subprocess.run([exe, str(CASES)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last == f"n={CASES}: E mismatches 0, non-zero skipped terms 0, guard violations 0", last
    # every kind of case that can skip did, and the margin was approached from both sides
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("kind ")]
    skipped = {int(row[1]): int(row[-1]) for row in rows}
    assert all(skipped[k] > 0 for k in (0, 1, 2, 3, 4, 5)), skipped
    assert skipped[6] == 0 and skipped[7] == 0, skipped
