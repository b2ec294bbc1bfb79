"""flx_scene_upload_device without a GPU: where it is declared and bound, that capi still imports without torch, and the table of refusals its kernel implements
(scene_upload_device_util.offences: a key entry * 4 + rule per offence, the least key decides) against hand-written cases and against the text of the host loop it
stands in for (csrc/flx_scene.hip).  tests/test_scene_upload_device_gpu.py runs the two calls beside each other."""
import os
import re
import subprocess
import sys

import numpy as np

import synth_scene
from scene_upload_device_util import (MESSAGES, POSITIONS, REFUSAL_ENTRIES, SKIP, TRANSFORM, TYPE, last_box_reaches_the_end, offences, offend, overlapping_boxes,
                                      refusal, terminator_in_the_middle)

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
    text = read(*SCENE_HIP)
    start = text.index('extern "C" flx_status %s(' % name)
    return text[start:text.index('\nextern "C"', start + 1)]


def static_body_of(name):
    text = read(*SCENE_HIP)
    start = text.index("static flx_status %s(" % name)
    return text[start:text.index("\n}\n", start)]


def test_the_library_exports_it_and_capi_binds_it():
    from flexlight_hip import capi
    assert "flx_scene_upload_device" in capi.EXPORTS
    assert hasattr(capi.LIB, "flx_scene_upload_device") and hasattr(capi.Context, "upload_scene_device")
    assert capi.LIB.flx_scene_upload_device.argtypes is not None and len(capi.LIB.flx_scene_upload_device.argtypes) == 7


def test_it_is_declared_beside_flx_scene_update_device_and_not_in_the_boundary_header():
    assert "flx_scene_upload_device" in declared("flexlight_hip_debug.h")
    assert "flx_scene_upload_device" not in declared("flexlight_hip.h")
    text = read("include", "flexlight_hip_debug.h")
    assert text.index("flx_status flx_scene_update_device(") < text.index("flx_status flx_scene_upload_device(") < text.index("flx_status flx_debug_scene_read(")


def test_capi_imports_without_torch():
    code = "import sys; sys.modules['torch'] = None; sys.path.insert(0, %r); from flexlight_hip import capi; print(capi.Context.upload_scene_device.__name__)" % PKG
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "upload_scene_device"


def test_the_messages_are_the_host_calls_in_the_host_calls_order():
    text = read(*SCENE_HIP)
    table = text[text.index("SCENE_UPLOAD_REFUSAL[3] = {"):]
    assert tuple(re.findall(r'"([^"]*)"', table[:table.index("};")])) == MESSAGES             # the one table, in the order of the kernel's rule numbers
    rules = text[text.index("enum UploadRule {"):]
    assert re.findall(r"\w+", rules[rules.index("{"):rules.index("}")]) == ["UPLOAD_RULE_TRANSFORM", "UPLOAD_RULE_SKIP", "UPLOAD_RULE_TYPE"]
    host = body_of("flx_scene_upload")
    loop = host[host.index("for (uint32_t i = 0; i < n_entries_padded; i++)"):host.index("flx_status s;")]
    assert loop.count("fail(") == 3
    assert re.findall(r"fail\(ctx, FLX_ERR_INVALID, SCENE_UPLOAD_REFUSAL\[UPLOAD_RULE_(\w+)\]\)", loop) == ["TRANSFORM", "SKIP", "TYPE"]      # as the loop meets them
    device = body_of("flx_scene_upload_device")
    assert "fail(ctx, FLX_ERR_INVALID, SCENE_UPLOAD_REFUSAL[rule < 3u ? rule : 2u])" in device and "rule = ~rec[0] & 3u" in device
    for message in MESSAGES:
        assert text.count(message) == 1
    # what is refused before an entry is looked at: one function holds the statuses and texts, in this order, and both calls begin with it
    checks = re.findall(r'fail\(ctx, (FLX_ERR_[A-Z_]+), "([^"]*)"\)', static_body_of("upload_refused"))
    assert checks == [("FLX_ERR_INVALID", "flx_scene_upload: empty scene"), ("FLX_ERR_INVALID", "flx_scene_upload: ids is NULL"),
                      ("FLX_ERR_INVALID", "flx_scene_upload: more than 2^28 - 1 entries")]
    for body in (host, device):
        before = body[:body.index("hipSetDevice")]
        assert "upload_refused(ctx, " in before and 'fail(ctx, FLX_ERR_INVALID, "' not in before


def base():
    return synth_scene.make_sized(REFUSAL_ENTRIES, 3, seed=7).arrays["geometry"].reshape(-1, 12)[:REFUSAL_ENTRIES].copy()


def test_the_table_takes_what_the_flatten_emits():
    for entries, transforms in ((7, 1), (300, 3), (5000, 3)):
        assert offences(synth_scene.make_sized(entries, transforms).arrays["geometry"]) == set()
    for scene in (terminator_in_the_middle(), last_box_reaches_the_end(), overlapping_boxes()):
        assert refusal(scene.arrays["geometry"]) is None


def test_the_table_refuses_hand_written_cases():
    n = REFUSAL_ENTRIES
    box = int(np.flatnonzero(base()[:, 10] == 1)[3])
    cases = [                                                       # (entry, word, value) -> rule
        ((5, 9, -1.0), TRANSFORM), ((5, 9, 1048576.0), TRANSFORM), ((5, 9, np.nan), TRANSFORM), ((5, 9, np.inf), TRANSFORM),
        ((box, 6, -1.0), SKIP), ((box, 6, float(n - box)), SKIP), ((box, 6, np.nan), SKIP), ((box, 6, np.inf), SKIP), ((box, 6, 1e30), SKIP),
        ((5, 10, 3.0), TYPE), ((5, 10, -1.0), TYPE), ((5, 10, 1.5), TYPE), ((5, 10, np.nan), TYPE), ((5, 10, np.inf), TYPE),
    ]
    for (entry, word, value), rule in cases:
        g = base()
        g[entry, word] = value
        assert offences(g) == {entry * 4 + rule}, (entry, word, value)
        assert refusal(g) == MESSAGES[rule]
    # what is NOT refused: the borders of the ranges, fractions, a terminator's free words, -0
    g = base()
    g[5, 9], g[6, 9] = 1048575.0, -0.0
    g[box, 6] = float(n - box - 1)
    g[box + 1, 9] = 1.5
    assert offences(g) == set()
    g = np.concatenate([base(), np.zeros((4, 12), np.float32)])
    g[n:, 6], g[n:, 9], g[n:, 0] = 1e9, -5.0, np.nan
    assert offences(g) == set()


def test_the_first_entry_decides_and_within_it_the_hosts_first_rule():
    for rule in (TRANSFORM, SKIP, TYPE):
        for position in POSITIONS:
            at = REFUSAL_ENTRIES - 1 if position == "last" else position
            g = base()
            offend(g, at, rule)
            assert offences(g) == {at * 4 + rule}
            later, earlier_rule = at + 37, (rule + 2) % 3
            if later < REFUSAL_ENTRIES:
                offend(g, later, earlier_rule)
                assert offences(g) == {at * 4 + rule, later * 4 + earlier_rule}
            assert refusal(g) == MESSAGES[rule], (rule, position)
    g = base()
    g[9, 9], g[9, 10] = -1.0, 3.0                                   # two rules in one entry: the transform number comes first
    assert offences(g) == {9 * 4 + TRANSFORM, 9 * 4 + TYPE} and refusal(g) == MESSAGES[TRANSFORM]
    g[9, 10], g[9, 6] = 1.0, -1.0
    assert offences(g) == {9 * 4 + TRANSFORM, 9 * 4 + SKIP} and refusal(g) == MESSAGES[TRANSFORM]
