"""flx_scene_update_device without a GPU: where it is declared and bound, that capi still imports without torch, and the table of refusals its kernel implements
(scene_update_device_util.offences: a key row * 4 + rule per offence, the least key decides) against the host call it stands in for.  flx_scene_update needs a
context, hence a GPU, so here its messages and their order are read from its source text (csrc/flx_scene.hip); tests/test_scene_update_device_gpu.py runs the
two calls beside each other."""
import os
import re
import subprocess
import sys

import numpy as np

import synth_scene
from scene_update_device_util import FINITE, KIND, MESSAGES, POSITIONS, SKIP, SPAN, TRANSFORM, is_box, is_triangle, offences, refusal, refusal_cases, span_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "web-ray-tracer_amd")


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", read("include", header), flags=re.S)
    return set(re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", text))


SCENE_HIP = ("web-ray-tracer_amd", "csrc", "flx_scene.hip")


def body_of(name):
    """the text of the C function `name` in flx_scene.hip, up to the next function of the C ABI"""
    text = read(*SCENE_HIP)
    start = text.index('extern "C" flx_status %s(' % name)
    return text[start:text.index('\nextern "C"', start + 1)]


def static_body_of(name):
    """the text of the file's own function `name`, up to its closing brace"""
    text = read(*SCENE_HIP)
    start = text.index("static flx_status %s(" % name)
    return text[start:text.index("\n}\n", start)]


def test_the_function_is_declared_beside_flx_scene_update_and_not_in_the_boundary_header():
    assert "flx_scene_update_device" in declared("flexlight_hip_debug.h")
    assert "flx_scene_update_device" not in declared("flexlight_hip.h")
    text = read("include", "flexlight_hip_debug.h")
    assert text.index("flx_status flx_scene_update(") < text.index("flx_status flx_scene_update_device(") < text.index("flx_status flx_debug_scene_read(")


def test_capi_exports_it():
    from flexlight_hip import capi
    assert "flx_scene_update_device" in capi.EXPORTS
    assert hasattr(capi.LIB, "flx_scene_update_device") and hasattr(capi.Context, "update_scene_rows_device")


def test_capi_imports_without_torch():
    code = "import sys; sys.modules['torch'] = None; sys.path.insert(0, %r); from flexlight_hip import capi; print(capi.Context.update_scene_rows_device.__name__)" % PKG
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "update_scene_rows_device"


def test_the_messages_are_the_host_calls_in_the_host_calls_order():
    text = read(*SCENE_HIP)
    table = text[text.index("SCENE_UPDATE_REFUSAL[4] = {"):]
    assert tuple(re.findall(r'"([^"]*)"', table[:table.index("};")])) == MESSAGES             # the one table, in the order of the kernel's rule numbers
    rules = text[text.index("enum UpdateRule {"):]
    assert re.findall(r"\w+", rules[rules.index("{"):rules.index("}")]) == ["UPDATE_RULE_KIND", "UPDATE_RULE_TRANSFORM", "UPDATE_RULE_SKIP", "UPDATE_RULE_FINITE"]
    host = body_of("flx_scene_update")
    loop = host[host.index("for (uint32_t r = 0; r < n_entries; r++)"):host.index("FLX_HIP(ctx, hipSetDevice")]
    assert loop.count("fail(") == 4
    assert re.findall(r"fail\(ctx, FLX_ERR_INVALID, SCENE_UPDATE_REFUSAL\[UPDATE_RULE_(\w+)\]\)", loop) == ["KIND", "TRANSFORM", "SKIP", "FINITE"]      # as the loop meets them
    device = body_of("flx_scene_update_device")
    assert "fail(ctx, FLX_ERR_INVALID, SCENE_UPDATE_REFUSAL[verdict & 3u])" in device
    for message in MESSAGES:
        assert text.count(message) == 1
    # what is refused before a row is looked at: one function holds the statuses and texts, in this order, and both calls begin with it
    checks = re.findall(r'fail\(ctx, (FLX_ERR_[A-Z_]+), "([^"]*)"\)', static_body_of("update_refused"))
    assert checks == [("FLX_ERR_NO_SCENE", "flx_scene_update before flx_scene_upload"), ("FLX_ERR_INVALID", "flx_scene_update: the rows leave the entry array"),
                      ("FLX_ERR_INVALID", "flx_scene_update: geometry is NULL"),
                      ("FLX_ERR_INVALID", "flx_scene_update: the uploaded scene has a NaN vertex (its boxes cannot be refitted as the flatten makes them)")]
    for body in (host, device):
        assert 0 < body.index("update_refused(ctx, first_entry, n_entries, ") < body.index("hipSetDevice")
        assert 'fail(ctx, FLX_ERR_INVALID, "flx_scene_update:' not in body and "FLX_ERR_NO_SCENE" not in body


def test_the_table_refuses_the_cases_and_takes_the_lowest_key():
    g = synth_scene.make_sized(5000, 3, seed=5).arrays["geometry"].reshape(-1, 12)
    assert refusal(g, 0, g) is None and offences(g, 700, g[700:1000]) == set()
    cases = refusal_cases()
    assert len(cases) == 4 + 27
    for name, (wanted, change, rule) in cases.items():
        for position in POSITIONS:
            first, at = span_with(g, wanted, position)
            rows = g[first:first + SPAN].copy()
            rows[at] = change(rows[at])
            assert offences(g, first, rows) == {at * 4 + rule}, (name, position)
            assert refusal(g, first, rows) == MESSAGES[rule]
    # two rows: the lower row's rule, whatever its number
    first, at = span_with(g, lambda g: is_triangle(g) & np.roll(g[:, 10] != 0, -2), 20)
    rows = g[first:first + SPAN].copy()
    rows[at, 8], rows[at + 2, 10] = np.nan, 3.0 - rows[at + 2, 10]
    assert min(offences(g, first, rows)) == at * 4 + FINITE and refusal(g, first, rows) == MESSAGES[FINITE]
    # two rules in one row: the host's first
    rows = g[first:first + SPAN].copy()
    rows[at, 0], rows[at, 9] = np.inf, rows[at, 9] + 1
    assert offences(g, first, rows) == {at * 4 + TRANSFORM, at * 4 + FINITE} and refusal(g, first, rows) == MESSAGES[TRANSFORM]
    rows[at, 10] = 1.0                                      # now a box by its own word: its vertices are not looked at, its word 6 is (and stands)
    assert offences(g, first, rows) == {at * 4 + KIND, at * 4 + TRANSFORM} and refusal(g, first, rows) == MESSAGES[KIND]
    first, at = span_with(g, is_box, 100)
    rows = g[first:first + SPAN].copy()
    rows[at, :6], rows[at, 6] = np.nan, rows[at, 6] + 1     # a box's six floats are not vertices
    assert offences(g, first, rows) == {at * 4 + SKIP}
    # a terminator's words 6 and 9 are free
    dead = int(np.flatnonzero(g[:, 10] == 0)[0])
    rows = g[dead:dead + 1].copy()
    rows[0, 6], rows[0, 9], rows[0, 0] = 7.0, 5.0, np.nan
    assert offences(g, dead, rows) == set()
