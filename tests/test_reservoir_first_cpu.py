"""Does the reservoir take the first light it weighs?  include/flx_reservoir_first.h answers from the ARGUMENT of the sine behind the draw and from the weight — an f32
range check where reservoirPick (csrc/flx_device.h) made two sines in double — and the shading of the persistent kernels uses that answer in scenes of one light
(FLX_SHADE_FIRST_LIGHT).  tests/reservoir_first_main.c, a stand-alone C program, holds the rule against the literal flx_abs(y) * w <= w with y from flx_sin:

  * the argument float by float on both sides of +2^20 and -2^20, NaN, the infinities, zeros, denormals, multiples of pi (where y may be 0);
  * every weight of +0, the smallest and the largest denormal, the smallest normal, 1, FLT_MAX, +inf, NaN, and ordinary ones;
  * 200 000 random (z, w, seed) triples through noise()'s own operations, seeds on both sides of the one at which the argument passes 2^20.

It is compiled with the host compiler as the oracle is (-ffp-contract=off), once plain and once with the address and undefined-behaviour sanitizers, and run directly.
There may be no disagreement."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function"]


@pytest.mark.parametrize("name,extra", [("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])])
def test_the_rule_is_the_literal_comparison(tmp_path, name, extra):
    exe = str(tmp_path / ("reservoir_first_" + name))
    subprocess.check_call(["gcc"] + CFLAGS + extra + ["-I", os.path.join(ROOT, "include"), os.path.join(HERE, "reservoir_first_main.c"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    m = re.search(r"checked (\d+) pairs \((\d+) random triples\): the literal test is true in (\d+), takes the sine in the rule's slow branch in (\d+); disagreements (\d+)", run.stdout)
    assert m, run.stdout
    checked, triples, taken, slow, disagreed = (int(g) for g in m.groups())
    assert disagreed == 0
    assert triples >= 100000 and checked >= triples + 2 * 8193 * 6
    assert 0 < taken < checked and slow > 0          # both answers occur, and the branch of a weight of +inf ran
