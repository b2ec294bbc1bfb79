"""The temporal accumulation pass for any history depth, from the reference's text alone, and a host-side ring to drive it.

temporal_literal is the shader that modules/pathtracerWGL2.js:571-662 GENERATES for config.temporalSamples = ring.depth, and TemporalRing the four lists of
RGBA8 history textures the host rotates before every frame (:389-402), both evaluated one float32 operation at a time in the shader's order, over whole
planes at once.  It is the any-depth, vectorised form of tests/analysis/make_temporal_kat.py's scalar temporal_shader (which is hard-wired to a depth of 4)
with make_filter_kat.py's pins: an RGBA8 store is 0 for not (x > 0), 255 for x >= 1, else int(f32(f32(x * 255) + 0.5)); a fetch is byte / 255; pow is
computed in float64 and rounded once.  Nothing here is taken from oracle/ or from the library: tests hold both against it.

The pass reads and writes the texel of its own pixel only, so planes are [rows, W, 4] in any row order (top-down frames and a context's packed strips alike).

Coverage tallies, from the masks temporal_literal returns, what a run of frames asked of the pass: tests assert it so that a sequence in which every
history slot matches every pixel (a still camera over a still scene) cannot pass for a test of the id comparison.
"""
import numpy as np

f32 = np.float32
GBUFFER_OF_RING = (("c", "color"), ("ip", "color_ip"), ("id", "location_id"), ("oid", "original_id"))      # TempTexture, TempIpTexture, TempIdTexture, TempOriginalIdTexture

# which of a run's camera positions frame f is traced from: no period, three positions, runs of equal and of alternating positions
SCHEDULE = (0, 1, 0, 0, 1, 1, 0, 2, 1, 0, 2, 2, 0, 1, 2, 0, 0, 2, 1, 1, 0, 1, 2, 2)
STEP = 0.05                                                                # of camera[0] per position


def effective_depth(temporal_samples):
    """config.temporalSamples as the library reads flx_frame_params.temporal_samples: 0 (and below) means 4, above 16 means 16"""
    return 4 if temporal_samples <= 0 else min(int(temporal_samples), 16)


def quantise(plane):
    """float plane -> the bytes an RGBA8 render target stores (make_filter_kat.py's Tex.store)"""
    x = np.asarray(plane, f32)
    low, high = ~(x > 0), x >= 1                                           # (NaN: not > 0)
    with np.errstate(all="ignore"):
        q = (np.where(low | high, f32(0), x) * f32(255) + f32(0.5)).astype(f32)
    return np.where(low, 0, np.where(high, 255, q.astype(np.int32))).astype(np.uint8)


def fetch(plane_u8):
    """texelFetch of an RGBA8 texture"""
    return plane_u8.astype(f32) / f32(255)


class TemporalRing:
    """TempTexture, TempIpTexture, TempIdTexture, TempOriginalIdTexture: `depth` zeroed planes each; slot 0 is the frame just traced"""

    def __init__(self, depth, rows, W):
        self.depth, self.rows, self.W = int(depth), int(rows), int(W)
        self.c, self.ip, self.id, self.oid = ([np.zeros((rows, W, 4), np.uint8) for _ in range(depth)] for _ in range(4))
        self.pushed = 0

    def push(self, gbuffers):
        """renderFrame's rotation, unshift(pop()), then the path-trace pass renders into slot 0"""
        for ring, name in GBUFFER_OF_RING:
            planes = getattr(self, ring)
            planes.insert(0, planes.pop())
            q = quantise(gbuffers[name])
            assert q.shape == (self.rows, self.W, 4), (name, q.shape)
            planes[0] = q
        self.pushed += 1

    @property
    def filled(self):
        """how many of the history slots 1 .. depth - 1 hold a frame (the others are still zero)"""
        return min(self.pushed, self.depth) - 1


class Masks:
    """per visited history slot (slots 1 .. 4 * groups; [k] is slot k + 1, the ones >= depth are vec4(0) stand-ins): where its location id / its original id
    equalled the new frame's, bool [slots, rows, W]; counter / glass_counter: the float32 planes the sums were divided by"""

    def __init__(self, id_match, oid_match, counter, glass_counter):
        self.id, self.oid, self.counter, self.glass_counter = id_match, oid_match, counter, glass_counter


def temporal_literal(ring, hdr, use_filter):
    """the generated shader for ring.depth over every texel -> (canvas float32 [rows, W, 4], or with use_filter the two uint8 planes (dColor, dIp) the pass
    renders into RenderTexture[0] / IpRenderTexture[0]; Masks)"""
    N = ring.depth
    ident, originalId = fetch(ring.id[0]), fetch(ring.oid[0])             # vec4 id, originalId
    shape = ident.shape[:2]
    counter = np.full(shape, f32(1.0))
    glassCounter = np.full(shape, f32(1.0))
    c0, i0 = fetch(ring.c[0]), fetch(ring.ip[0])
    centerW = c0[..., 3]
    color = c0[..., :3] + i0[..., :3] * f32(256.0)
    glassFilter = i0[..., 3].copy()
    zero = np.zeros(ident.shape, f32)
    id_match, oid_match = [], []
    for i in range(1, N, 4):                                               # for (let i = 1; i < temporalSamples; i += 4): one mat4 of each ring
        slots = range(i, i + 4)
        c = [fetch(ring.c[j]) if j < N else zero for j in slots]
        ip = [fetch(ring.ip[j]) if j < N else zero for j in slots]
        ids = [fetch(ring.id[j]) if j < N else zero for j in slots]
        oids = [fetch(ring.oid[j]) if j < N else zero for j in slots]
        for k in range(4):                                                 # if (id_i[k].xyzw == id.xyzw)
            m = (ids[k] == ident).all(axis=-1)
            color = np.where(m[..., None], color + (c[k][..., :3] + ip[k][..., :3] * f32(256.0)), color)
            counter = np.where(m, counter + f32(1.0), counter)
            id_match.append(m)
        for k in range(4):                                                 # if (originalId_i[k].xyzw == originalId.xyzw)
            m = (oids[k] == originalId).all(axis=-1)
            glassFilter = np.where(m, glassFilter + ip[k][..., 3], glassFilter)
            glassCounter = np.where(m, glassCounter + f32(1.0), glassCounter)
            oid_match.append(m)
    color = color / counter[..., None]
    glassFilter = glassFilter / glassCounter
    none = np.zeros((0,) + shape, bool)
    masks = Masks(np.array(id_match) if id_match else none, np.array(oid_match) if oid_match else none, counter, glassCounter)
    assert color.dtype == f32 and glassFilter.dtype == f32
    if use_filter:
        mod1 = color - f32(1.0) * np.floor(color / f32(1.0))              # mod(color, 1.0)
        dColor = quantise(np.concatenate([mod1, centerW[..., None]], axis=-1))
        dIp = quantise(np.concatenate([np.floor(color) / f32(256.0), glassFilter[..., None]], axis=-1))
        return (dColor, dIp), masks
    if hdr == 1:
        with np.errstate(all="ignore"):
            color = color / (color + f32(1.0))
            inv_gamma = f32(1.0) / f32(0.8)
            color = np.power((f32(4.0) * color).astype(np.float64), np.float64(inv_gamma)).astype(f32) / f32(4.0) * f32(1.3)
    return np.concatenate([color, centerW[..., None]], axis=-1).astype(f32), masks


class Coverage:
    """what a run of frames asked of the id comparisons, tallied from the literal's masks frame by frame"""

    def __init__(self, depth):
        self.depth = depth
        self.patterns = set()              # (filled, which of the filled slots matched) among covered pixels
        self.partial = 0                   # covered pixel-frames whose filled slots match partly: some, not all
        self.id_miss_oid_hit = 0           # filled slot-pixels whose location id differs while the original id is equal
        self.uncovered_stand_in = 0        # uncovered pixels (zero id) counted for a vec4(0) stand-in slot
        self.counters = set()              # values the colour sum was divided by

    def add(self, ring, masks):
        filled = ring.filled
        covered = (ring.id[0] != 0).any(axis=-1)
        idm, oidm = masks.id[:filled], masks.oid[:filled]
        if filled:
            hits = idm.sum(axis=0)
            partly = covered & (hits > 0) & (hits < filled)
            self.partial += int(partly.sum())
            bits = (idm.astype(np.int64) << np.arange(filled)[:, None, None]).sum(axis=0)
            self.patterns |= {(filled, int(b)) for b in np.unique(bits[covered])}
            self.id_miss_oid_hit += int((~idm & oidm).sum())
        stand_ins = masks.id[ring.depth - 1:]
        self.uncovered_stand_in += int((stand_ins & ~covered).sum())
        self.counters |= {int(v) for v in np.unique(masks.counter)}

    def figures(self):
        return "depth %d: %d match patterns, %d partly matching pixel-frames, %d id-miss / original-id-hit slot-pixels, %d uncovered stand-in matches, counters %s" % (
            self.depth, len(self.patterns), self.partial, self.id_miss_oid_hit, self.uncovered_stand_in, sorted(self.counters))

    def check(self, uncovered):
        """the conditions a motion run has to meet (conditions on the test's inputs, not tolerances); uncovered: the scene leaves pixels of the frame uncovered"""
        what = self.figures()
        assert len(self.patterns) >= 8, what
        assert self.partial >= 100, what
        assert self.id_miss_oid_hit >= 100, what
        assert set(range(1, self.depth + 1)) <= self.counters, what
        if uncovered:
            assert self.uncovered_stand_in >= 1, what


def copy_params(p, **kw):
    q = type(p).from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def temporal_params(sc, w, h, temporal_samples, hdr=0, use_filter=0, spp=1, bounces=2, tile=(0, 0, 0)):
    p = sc.frame_params(width=w, height=h, samples=spp, max_reflections=bounces, use_filter=use_filter, hdr=hdr, tile=tile)
    p.is_temporal, p.temporal_samples = 1, temporal_samples
    return p


def still_frames(p, n_frames=None):
    """effective_depth + 3 frames of a still camera, frame f with the seed f % depth (pathtracerWGL2.js:291, 347)"""
    depth = effective_depth(p.temporal_samples)
    return [copy_params(p, random_seed=float(f % depth)) for f in range(depth + 3 if n_frames is None else n_frames)]


def motion_frames(p, n_frames=None, step=STEP):
    """the same run with the camera at position SCHEDULE[f] * step along x in frame f"""
    frames = still_frames(p, n_frames)
    assert len(frames) <= len(SCHEDULE)
    for f, q in enumerate(frames):
        q.camera[0] = p.camera[0] + f32(SCHEDULE[f] * step)
    return frames


def far_frames(sc, p, far=200.0, n_frames=None):
    """still_frames with the camera moved back 20 * (far - 1) along its viewing direction and zoomed in `far` times (the scene keeps about its size in the frame).  The location id is
    mod(position, div) / div with div twice the distance to the camera (fragment:640-642): from far away its x, y, z store as the byte 0 wherever the
    position's coordinates are positive, and only w = 1 / 255 tells such a covered pixel from a zero texel — an empty history slot or a vec4(0) stand-in."""
    from flexlight_hip.scene_io import view_matrix
    cam = sc.meta["camera"]
    forward = np.array([-np.sin(cam["fx"]) * np.cos(cam["fy"]), -np.sin(cam["fy"]), np.cos(cam["fx"]) * np.cos(cam["fy"])])      # the view matrix' third row
    q = copy_params(p)
    for k in range(3):
        q.camera[k] = p.camera[k] - float(forward[k]) * 20.0 * (far - 1.0)
    q.view_matrix[:] = view_matrix(cam["fx"], cam["fy"], cam["fov"] / far, p.width, p.height).tolist()
    return still_frames(q, n_frames)


def only_w_tells(gbuffers):
    """covered pixels whose stored location id is (0, 0, 0, w): bool [rows, W]"""
    q = quantise(gbuffers["location_id"])
    return (q[..., :3] == 0).all(axis=-1) & (q[..., 3] != 0)


def literal_run(depth, gbuffers_of_frames, hdr, use_filter=0, coverage=None):
    """push every frame's G-buffers into a fresh ring -> the literal's result per frame"""
    ring, out = None, []
    for gb in gbuffers_of_frames:
        if ring is None:
            rows, W = gb["color"].shape[:2]
            ring = TemporalRing(depth, rows, W)
        ring.push(gb)
        res, masks = temporal_literal(ring, hdr, use_filter)
        if coverage is not None:
            coverage.add(ring, masks)
        out.append(res)
    return out
