"""A context gives back the device memory it took: every buffer of flx_context is owned by the context and goes with it
(csrc/flx_context.h: Buffer), whatever pipelines, passes and loops the context ran."""
import pytest

pytestmark = pytest.mark.gpu

GRANULE = 2 << 20                  # the device allocator's granule: the slack of the comparison below


def exercise(ctx, sc):
    """each kind of frame once, so that every workspace of the context has been allocated — at 1280 x 720, where the smallest buffer of a frame
    (an RGBA8 plane, 3.5 MiB) is larger than the comparison's slack"""
    p = sc.frame_params(width=1280, height=720, samples=2, max_reflections=3, use_filter=0)
    ctx.update_scene(sc)
    for pipeline in (1, 2, 3):                                  # per pixel, persistent paths, wavefront
        ctx.set_pipeline(pipeline)
        frame = ctx.render(p)[0]
        assert ctx.last_pipeline() == pipeline
    ctx.set_pipeline(0)
    f = sc.frame_params(width=1280, height=720, samples=2, max_reflections=3, use_filter=1)
    ctx.render(f)                                               # the denoise chain
    f.is_temporal = 1
    ctx.render(f)                                               # the temporal rings
    ctx.fxaa(frame)
    ctx.taa(frame)
    ctx.raster_render(p)
    ctx.set_frame_chain(0)                                      # two lanes: the second one's context and workspace
    ctx.frame_begin(p, rgba8=True)
    ctx.frame_begin(p)
    bytes8, floats = ctx.frame_end()[0], ctx.frame_end()[0]
    assert bytes8.dtype.itemsize == 1 and floats.dtype.itemsize == 4
    ctx.set_frame_chain(3)                                      # the frame server
    ctx.frame_begin(p)
    assert ctx.last_chained() == 3
    ctx.frame_end()


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def context_cost(capi, work=None):
    """device memory that is gone after a context was made, used (work) and destroyed"""
    before = free_bytes()
    ctx = capi.Context(0)
    try:
        if work:
            work(ctx)
    finally:
        ctx.close()
    return before - free_bytes()


def test_a_context_that_rendered_gives_its_memory_back(scenes):
    """Free device memory before a context that ran every pipeline, the filter and temporal passes, FXAA and TAA, the rasterizer, the two lanes
    of the frame loop in both formats and the frame server — and after its destruction: no more is gone than after an idle context
    (made and destroyed first, in this process: what the runtime keeps for itself), give or take one allocation granule.

    Contexts of their own ran the same frames before either reading, so that what the runtime makes once per process and keeps — the
    kernels' code objects, its hardware queues, their scratch — is there already: in a fresh process the first such context is followed by
    504 MiB less free memory and the second by 160 MiB less, whichever library version runs, every later one by none (a process opens four
    hardware queues, and successive contexts' streams come to lie on different ones; hence four).  A buffer that a context does not free is
    lost with every context, the measured one included."""
    from flexlight_hip import capi
    sc = scenes("dragon")
    for _ in range(4):
        context_cost(capi, lambda ctx: exercise(ctx, sc))
    idle = context_cost(capi)
    used = context_cost(capi, lambda ctx: exercise(ctx, sc))
    print("device memory gone after an idle context: %d bytes, after one that rendered: %d bytes" % (idle, used))
    assert used <= max(idle, 0) + GRANULE, (used, idle)
