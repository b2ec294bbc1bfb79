"""GPU frames against literal WHOLE PIXELS (tests/golden/pixel_kat.json.gz, tests/analysis/make_pixel_kat.py: lightTrace with all its bounces and main(),
fragment:464-646, run from the shader text over the reference's arrays; the primary hit is the one input that is not from the text): every pipeline's colour
without the filter, and the five G-buffers the filter frame's trace kernel writes — bit for bit, without the oracle in between."""
import numpy as np
import pytest

from test_oracle_kat import _pixel_kat_cases, assert_pixel_kat, pixel_kat_expectations

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(len(_pixel_kat_cases())))
def test_whole_pixels_literal(hip, scenes, k):
    case = _pixel_kat_cases()[k]
    sc, p, rows, want_color, want_gb = pixel_kat_expectations(case, scenes)
    hip.update_scene(sc)
    try:
        # the per-pixel kernel twice — a pixel's samples side by side (k_trace_samples, where the frame allows it) and one after the other (k_trace_pixels) —,
        # with the filter's outputs and without
        for pipeline, organisation, front, sample_parallel in ((1, 0, 1, 1), (1, 0, 1, 0), (2, 0, 1, 1), (3, 1, 0, 1), (3, 2, 0, 1), (3, 2, 2, 1), (3, 1, 3, 1), (0, 0, 1, 1)):
            hip.set_pipeline(pipeline)
            hip.set_wavefront_organisation(organisation)
            hip.set_frame_front(front)
            hip.set_sample_parallel(sample_parallel)
            gbs = {}
            if pipeline == 1:
                p.use_filter = 1
                _, _, gbs = hip.render(p, gbuffers=True)
                p.use_filter = 0
            frame, _, _ = hip.render(p)
            what = "GPU pipeline %d organisation %d front %d sample_parallel %d, case %d" % (pipeline, organisation, front, sample_parallel, k)
            if pipeline == 1:
                ts = hip.last_trace_kernel()[0]
                assert ts == (case["samples"] if sample_parallel and case["samples"] in (2, 4, 8) and case["bounces"] <= 4 and (case["samples"], case["bounces"]) != (8, 4) else 0), (what, ts)
            assert_pixel_kat(case, rows, want_color, want_gb if pipeline == 1 else {}, frame, gbs, what)
    finally:
        hip.set_pipeline(0)
        hip.set_wavefront_organisation(0)
        hip.set_frame_front(1)
        hip.set_sample_parallel(1)
