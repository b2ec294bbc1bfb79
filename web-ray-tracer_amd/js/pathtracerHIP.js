'use strict';
/*
 * PathTracerHIP — the FlexLight renderer object whose frames are traced by libflexlight_hip.so on an
 * MI355X instead of by WebGL2.  It has the shape FlexLight expects from a renderer
 * (reference modules/pathtracerWGL2.js:25-78,143,167,191; SURVEY.md §8b): type, public config /
 * camera / scene, fps, fpsLimit, canvas getter, async render(), halt(), async updateScene(),
 * async updatePrimaryLightSources() — plus renderFrame(), a synchronous single frame for headless use.
 * Conventions kept from the reference: config, camera and scene are re-read every frame; lights,
 * transforms and (when their list changed) atlases are re-derived every frame (pathtracerWGL2.js:
 * 258-262, 361-365); errors of the frame loop go to console.error, renderFrame() throws.
 * The "canvas" is any object with width and height; if it has onFrame(frame) the loop calls it.
 */
const path = require('path');
const { Transform } = require('./scene.js');
const sceneFile = require('./sceneFile.js');

let addon = null;
function native () {
  if (!addon) {
    const file = path.join(__dirname, '..', 'napi', 'flexlight_napi.node');
    try {
      addon = require(file);
    } catch (e) {
      throw new Error('flexlight_napi.node is not built or cannot load libflexlight_hip.so (' + e.message +
        '). Build with `python -c "import __graft_entry__ as g; g.build()"`. There is no CPU fallback.');
    }
  }
  return addon;
}

/* flx_rays_cast on a context whose scene, lights and transforms are up (both renderers' castRays): the hit rows as the library writes them, 8 words a ray
 * (include/flexlight_hip_debug.h), unpacked into typed arrays */
function castRaysOn (context, rays, what) {
  if (!(rays instanceof Float32Array) || rays.length % 8 !== 0) throw new TypeError('castRays: rays is a Float32Array of 8 floats per ray');
  const hits = native().castRays(context, rays, what === undefined ? 3 : what);
  const n = rays.length / 8;
  const words = new Uint32Array(hits), f = new Float32Array(hits), i32 = new Int32Array(hits);
  const out = { suv: new Float32Array(3 * n), entry: new Int32Array(n), transform: new Int32Array(n), occluded: new Uint8Array(n) };
  for (let k = 0; k < n; k++) {
    out.suv[3 * k] = f[8 * k]; out.suv[3 * k + 1] = f[8 * k + 1]; out.suv[3 * k + 2] = f[8 * k + 2];
    out.entry[k] = i32[8 * k + 3]; out.transform[k] = i32[8 * k + 4] >> 1; out.occluded[k] = words[8 * k + 5];
  }
  return out;
}

/* flx_rays_trace on a context whose scene, lights, transforms and atlases are up: the radiance rows as the library writes them, 8 words a ray
 * (include/flexlight_hip_debug.h), unpacked into typed arrays */
function traceRaysOn (context, rays, params, order, volume, gain) {
  if (!(rays instanceof Float32Array) || rays.length % 8 !== 0) throw new TypeError('traceRays: rays is a Float32Array of 8 floats per ray');
  const rows = volume ? native().traceRaysGather(context, rays, params, order, volume, gain)      // (volume: bakeVolume's native handle)
    : order ? native().traceRaysOrdered(context, rays, params, order) : native().traceRays(context, rays, params);      // (order: FLX_TRACE_ORDER_* bits)
  const n = rays.length / 8;
  const words = new Uint32Array(rows), f = new Float32Array(rows), i32 = new Int32Array(rows);
  const out = { radiance: new Float32Array(4 * n), s: new Float32Array(n), entry: new Int32Array(n), transform: new Int32Array(n), shades: new Uint32Array(n) };
  for (let k = 0; k < n; k++) {
    out.radiance[4 * k] = f[8 * k]; out.radiance[4 * k + 1] = f[8 * k + 1]; out.radiance[4 * k + 2] = f[8 * k + 2]; out.radiance[4 * k + 3] = f[8 * k + 3];
    out.s[k] = f[8 * k + 4]; out.entry[k] = i32[8 * k + 5]; out.transform[k] = i32[8 * k + 6] >> 1; out.shades[k] = words[8 * k + 7];
  }
  return out;
}

/* The planes of a surface call (flx_rays_surface, flx_frame_surface: include/flexlight_hip_debug.h "surface rows") as typed arrays over the buffer the library
 * wrote: per plane asked for a Float32Array of 4 floats a row — hit, position, geometryNormal, normal, uv, albedo, rme, tpo, in that bit order of `fields` — and
 * the two integer words as arrays of their own: entry (word 3 of hit, -1: none) and transform (word 2 of uv is 2 x the transform number). */
/* the projections of a camera description, in the order of FLX_CAMERA_* (include/flexlight_hip_debug.h "cameras") */
const CAMERA_PROJECTIONS = ['pinhole', 'panorama', 'fisheye', 'orthographic', 'cubeFace'];
/* a camera description: a plain object (not the Float32Array of rays the same argument may be) */
function isCameraDescription (x) { return x !== null && typeof x === 'object' && !ArrayBuffer.isView(x) && !Array.isArray(x); }

const SURFACE = { HIT: 1, POSITION: 2, GEOMETRY_NORMAL: 4, NORMAL: 8, UV: 16, ALBEDO: 32, RME: 64, TPO: 128, ALL: 255 };
const SURFACE_PLANES = ['hit', 'position', 'geometryNormal', 'normal', 'uv', 'albedo', 'rme', 'tpo'];
function unpackSurface (buffer, n, fields) {
  const out = { n, fields };
  let p = 0;
  SURFACE_PLANES.forEach((name, bit) => {
    if (!(fields >> bit & 1)) return;
    out[name] = new Float32Array(buffer, p * n * 16, 4 * n);
    const i32 = new Int32Array(buffer, p * n * 16, 4 * n);
    if (name === 'hit') { out.entry = new Int32Array(n); for (let k = 0; k < n; k++) out.entry[k] = i32[4 * k + 3]; }
    if (name === 'uv') { out.transform = new Int32Array(n); for (let k = 0; k < n; k++) out.transform[k] = i32[4 * k + 2] >> 1; }
    p++;
  });
  return out;
}
/* flx_rays_surface on a context whose scene, lights, transforms and atlases are up (both renderers' surfaceRays) */
function surfaceRaysOn (context, rays, fields, textureWidth) {
  if (!(rays instanceof Float32Array) || rays.length % 8 !== 0) throw new TypeError('surfaceRays: rays is a Float32Array of 8 floats per ray');
  const f = fields === undefined ? SURFACE.ALL : fields;
  return unpackSurface(native().surfaceRays(context, rays, f, textureWidth), rays.length / 8, f);
}

class PathTracerHIP {
  constructor (canvas, scene, camera, config, options) {
    this.type = 'pathtracer';
    this.config = config;
    this.camera = camera;
    this.scene = scene;
    this.fps = 0;
    this.fpsLimit = Infinity;
    this._canvas = canvas;
    this._device = (options && options.device) || 0;
    this._tile = (options && options.tile) || null;      // {rows, index, count}: this context's strips of the frame
    /* several GPUs in this process (SURVEY.md 8e; not in the reference, which has one WebGL2 context): devices: N = GPUs 0 .. N - 1,
     * or a list of device numbers (a number may repeat: a rehearsal on a one-GPU box).  The frame is cut into strips of tileRows
     * rows dealt round robin to the GPUs and gathered inside the library (flx_group_render: RCCL all-gather + reassembly).  With config.temporal
     * every GPU keeps the history of its own strips, and frames go through the group's frame loop (flx_group_frame_begin / _end). */
    const dv = options && options.devices;
    this._devices = Array.isArray(dv) ? dv.slice() : (dv > 1 ? Array.from({ length: dv }, (_, i) => i) : null);
    this._tileRows = (options && options.tileRows) || 8;
    this.present8 = !!(options && options.present8);     // the frame loop hands out the canvas' RGBA8 instead of float radiance
    this.groupLanes = 3;                                  // frames in flight of a group's frame loop (2 or 3)
    this._group = null;
    this._ctx = null;
    this._halt = true;
    this._atlasLists = [null, null, null];
    this._haveScene = false;
    this._temporalFrame = 0;                             // pathtracerWGL2.js:291,562
    this.lastFrame = null;
  }

  get canvas () { return this._canvas; }

  _context () {
    if (this._devices) throw new Error('this renderer drives a group of GPUs: per-context calls are not available');
    if (!this._ctx) this._ctx = native().createContext(this._device);
    return this._ctx;
  }

  /* the GPU(s) behind the renderer: one context or a group of them, the same four uploads and one render call */
  _gpu () {
    const n = native();
    if (this._devices) {
      if (!this._group) this._group = n.createGroup(this._devices);
      const g = this._group;
      return {
        uploadScene: (a, b, c) => n.groupUploadScene(g, a, b, c), updateSceneRows: (f, a, b) => n.groupUpdateSceneRows(g, f, a, b), uploadTransforms: (a, b) => n.groupUploadTransforms(g, a, b),
        uploadLights: a => n.groupUploadLights(g, a), uploadAtlas: (w, px, x, y) => n.groupUploadAtlas(g, w, px, x, y),
        uploadTextures: (w, list, x, y) => n.groupUploadTextures(g, w, list, x, y), updateTexture: (w, i, img) => n.groupUpdateTexture(g, w, i, img),
        render: (p, out, counters) => n.groupRender(g, [p], this._tileRows, out, counters),
        renderBatch: (ps, out, counters) => n.groupRender(g, ps, this._tileRows, out, counters),
        rows: p => p.height
      };
    }
    const c = this._context();
    return {
      uploadScene: (a, b, d) => n.uploadScene(c, a, b, d), updateSceneRows: (f, a, b) => n.updateSceneRows(c, f, a, b), uploadTransforms: (a, b) => n.uploadTransforms(c, a, b),
      uploadLights: a => n.uploadLights(c, a), uploadAtlas: (w, px, x, y) => n.uploadAtlas(c, w, px, x, y),
      uploadTextures: (w, list, x, y) => n.uploadTextures(c, w, list, x, y), updateTexture: (w, i, img) => n.updateTexture(c, w, i, img),
      render: (p, out, counters) => n.render(c, p, out, counters), renderBatch: (ps, out, counters) => n.renderBatch(c, ps, out, counters),
      rows: p => n.tileRowCount(p)
    };
  }

  get gpuInfo () {                                         // { size, rccl } of a group, { size: 1 } otherwise
    return this._devices ? native().groupInfo((this._gpu(), this._group)) : { size: 1, rccl: false };
  }

  halt () {                                               // pathtracerWGL2.js:70-77
    this._halt = true;
    if (this._pendingEnd) { this._releaseWhenIdle = true; return; }      // a frame is being waited for on a worker thread (render()'s frameEndAsync): released when it settles
    this._release();
  }

  _release () {
    if (this._ctx) {
      try { native().destroyContext(this._ctx); } catch (e) { console.warn('Unable to release the GPU context', e.message); }
      this._ctx = null;
      this._rayHistories = {};                            // the ray-image histories went with the context
    }
    if (this._group) {
      try { native().destroyGroup(this._group); } catch (e) { console.warn('Unable to release the GPU group', e.message); }
      this._group = null;
    }
    this._haveScene = false;
    this._built = null;
    this._atlasLists = [null, null, null];
    this._inFlight = 0;
    this._lanesSet = undefined;
  }

  /* The application moved something and says so (pathtracerWGL2.js:167-189).  Where only vertices and attributes moved — the same rows, kinds, skip counts,
   * transform numbers and ids as the arrays uploaded last (sceneFile.changedRows) — the changed rows go to the device, which refits the boxes itself
   * (flx_scene_update); anything else is the whole upload.  lastSceneUpload: 'full' | 'rows' | 'none' (nothing differed: nothing was sent). */
  async updateScene () {
    const built = await this.scene.generateArraysFromGraph();
    const rows = this._haveScene ? sceneFile.changedRows(this._built, built) : null;
    if (!rows) return this._uploadBuilt(built);
    if (rows.count > 0) {
      this._gpu().updateSceneRows(rows.first, built.geometryBuffer.subarray(rows.first * 12, (rows.first + rows.count) * 12),
        built.sceneBuffer.subarray(rows.first * 28, (rows.first + rows.count) * 28));
    }
    this._built = built;
    this.lastSceneUpload = rows.count > 0 ? 'rows' : 'none';
  }

  _uploadBuilt (built) {
    this._gpu().uploadScene(built.geometryBuffer, built.sceneBuffer, built.idBuffer);
    this._built = built;                                 // (what the device holds: the next updateScene() compares with it)
    this._haveScene = true;
    this.lastSceneUpload = 'full';
  }

  async updatePrimaryLightSources () {                    // pathtracerWGL2.js:143-165
    this._gpu().uploadLights(sceneFile.buildLightArray(this.scene));
  }

  _updateAtlases () {                                     // pathtracerWGL2.js:106-140: rebuild only when the list object or its members changed
    if (this.scene.prebuiltAtlases) {                    // a replayed scene (sceneFile.sceneFromFlxs): the atlases as they were built
      if (this._atlasLists[0] !== this.scene.prebuiltAtlases) {
        this.scene.prebuiltAtlases.forEach((a, which) => this._gpu().uploadAtlas(which, a.data, a.width, a.height));
        this._atlasLists = [this.scene.prebuiltAtlases, null, null];
      }
      return;
    }
    const lists = [this.scene.textures, this.scene.pbrTextures, this.scene.translucencyTextures];
    lists.forEach((list, which) => {
      const old = this._atlasLists[which];
      if (old && old.length === list.length && list.every((e, i) => e === old[i])) return;
      const sizes = this.scene.standardTextureSizes;
      this._atlasLists[which] = list.slice();
      if (list.length === 0) { this._gpu().uploadAtlas(which, null, 0, 0); return; }
      this._atlasLists[which].cells = [sizes[0], sizes[1]];      // what the resident atlas is built with (uploadTextures: the device resamples and composites, sceneFile.buildAtlas' bytes)
      if (old && old.cells && old.length === list.length && old.cells[0] === sizes[0] && old.cells[1] === sizes[1]) {
        list.forEach((e, i) => { if (e !== old[i]) this._gpu().updateTexture(which, i, sceneFile.nativeTexture(e)); });      // only the members that changed, each into its cell
      } else {
        this._gpu().uploadTextures(which, list.map(sceneFile.nativeTexture), sizes[0], sizes[1]);
      }
    });
  }

  frameParams (jitter) {                                  // pathtracerWGL2.js:307-347
    /* config.renderQuality scales the resolution the frame is traced at (pathtracerWGL2.js:264-267, 810-811: the canvas'
     * drawing buffer is clientWidth x renderQuality); the frame handed back has that size */
    const q = this.config.renderQuality > 0 ? this.config.renderQuality : 1;
    const w = Math.max(1, Math.round(this._canvas.width * q)), h = Math.max(1, Math.round(this._canvas.height * q));
    const cam = jitter ? Object.assign(Object.create(this.camera), { fx: this.camera.fx + jitter.x, fy: this.camera.fy + jitter.y }) : this.camera;
    const p = {
      width: w, height: h,
      camera: [this.camera.x, this.camera.y, this.camera.z],
      viewMatrix: Array.from(sceneFile.buildViewMatrix(cam, w, h)),                 // view rotation and TAA jitter (pathtracerWGL2.js:310-318)
      samples: this.config.samplesPerRay,
      maxReflections: this.config.maxReflections,
      minImportancy: this.config.minImportancy,
      useFilter: this.config.filter ? 1 : 0,
      isTemporal: this.config.temporal ? 1 : 0,
      temporalSamples: this.config.temporalSamples,
      hdr: this.config.hdr ? 1 : 0,
      ambient: [this.scene.ambientLight[0], this.scene.ambientLight[1], this.scene.ambientLight[2]],
      randomSeed: this.config.temporal ? this._temporalFrame : 0,          // pathtracerWGL2.js:347
      textureWidth: Math.floor(2048 / this.scene.standardTextureSizes[0])
    };
    if (this._tile) { p.tileRows = this._tile.rows; p.tileIndex = this._tile.index; p.tileCount = this._tile.count; }
    return p;
  }

  /* config.antialiasing (pathtracerWGL2.js:268-286): 'fxaa' | 'taa' | anything else = none.  TAA turns the camera by a sub-pixel
   * offset every frame (taa.js:120-127); the nine offsets sum to zero and are drawn once per renderer (taa.js:130-149) from
   * this.random, Math.random unless the application supplies its own. */
  _antialiasing () {
    const v = typeof this.config.antialiasing === 'string' ? this.config.antialiasing.toLowerCase() : undefined;
    const mode = (v === 'fxaa' || v === 'taa') ? v : undefined;
    if (mode !== this._aaMode) {
      this._aaMode = mode;
      this._taaNum = 0;
      if (mode === 'taa') { this._taaVecs = taaVectors(9, this.random || Math.random); if (this._ctx) native().taaReset(this._ctx); }
    }
    return mode;
  }

  _jitter () {                                            // taa.js:120-127
    this._taaNum = (this._taaNum + 1) % 9;
    const scale = 0.3 / Math.min(this._canvas.width, this._canvas.height);
    return { x: this._taaVecs[this._taaNum][0] * scale, y: this._taaVecs[this._taaNum][1] * scale };
  }

  /* One frame, synchronously.  Returns {width, height, rows, radiance: Float32Array(rows*width*4), frameMs, traceMs, counters?}. */
  /* scene arrays of this frame: scene once, then what the reference re-derives every frame (pathtracerWGL2.js:258-262, 361-365) */
  _uploadFrameState () {
    const gpu = this._gpu();
    if (!this._haveScene) this._uploadBuilt(this.scene.generateArraysFromGraph());
    this._updateAtlases();
    gpu.uploadLights(sceneFile.buildLightArray(this.scene));
    const tr = Transform.buildWGL2Arrays();
    gpu.uploadTransforms(tr[0], tr[1]);
    return gpu;
  }

  /* Rays of the application's own at the scene as the next frame would see it: picking, visibility (flx_rays_cast, include/flexlight_hip_debug.h "ray queries").
   * rays: Float32Array, 8 floats per ray — origin x y z, l (the length shadowTest compares; unused otherwise), direction x y z (not normalised: a hit lies at
   * origin + s * direction), one unused.  what: 1 the closest hit, 2 occluded within l (the renderer's own shadow predicate), 3 both.  Returns
   * { suv: Float32Array(3 n), entry: Int32Array(n) (the entry index in the flattened scene, -1: none), transform: Int32Array(n) (the transform number),
   * occluded: Uint8Array(n) }.  It waits for the answer; frames in flight finish unchanged. */
  castRays (rays, what) {
    if (this._devices) throw new Error('castRays: one GPU only (a group of GPUs casts no rays)');
    this._uploadFrameState();
    return castRaysOn(this._context(), rays, what);
  }

  /* What the renderer SEES along rays of the application's own: another projection (panorama, fisheye, orthographic, a stereo pair), light probes, reflection
   * rays of a hybrid renderer (flx_rays_trace, include/flexlight_hip_debug.h "ray queries").  rays: Float32Array, 8 floats per ray — origin x y z, noise x,
   * direction x y z (not normalised), noise y.  The two noise coordinates stand where a frame has the pixel's position in [-1, 1): rays with equal noise
   * coordinates draw equal random numbers, so give every ray its own.  options: { samples, maxReflections, minImportancy, ambient, randomSeed, textureWidth },
   * each by default what the next frame would use — config.samplesPerRay, config.maxReflections, config.minImportancy, scene.ambientLight, the texture width of
   * scene.standardTextureSizes — and seed 0.  Returns { radiance: Float32Array(4 n) (r g b and 1 for a hit; a miss is 0 0 0 0, not the ambient light),
   * s: Float32Array(n) (the first hit lies at origin + s * direction), entry: Int32Array(n) (-1: none), transform: Int32Array(n), shades: Uint32Array(n) (bounce
   * iterations shaded over all samples) }: per ray a frame's pixel without filter and temporal — the samples averaged, times the first surfaces' colour as the
   * LAST sample left it.  It waits for the answer; frames in flight finish unchanged.
   * options.order: 'hits' traces the rays in the order of their first hit points (flx_rays_trace_ordered) — the same rows, bit for bit and in the order given,
   * sooner where the rays come in no useful order: reflection rays, probe rays, shuffled rays.  Without it the rays are traced in the order given.  It is read
   * here and is no part of traceParams()'s result; any other value is a TypeError.
   * options.volume: bakeVolume's handle.  Every path then ends in the volume's irradiance at its last surface point times options.gain — by default
   * Math.fround(1 / Math.PI): irradiance over pi is the radiance a Lambertian surface sends on — where it ends in scene.ambientLight without (flx_rays_trace_gather,
   * "ray batches with a volume"): two bounces and a volume stand in for many bounces.  The handle's SH rows, its maps and its offsets stay on the device and are
   * honoured as renderIrradiance honours them; where the volume has nothing to say (no probe in reach, a path that shaded nothing) the ambient light stays.  A
   * volume that is no handle and a gain that is no number are TypeErrors.  Without options.volume the call is what it was. */
  traceRays (rays, options) {
    if (this._devices) throw new Error('traceRays: one GPU only (a group of GPUs traces no rays)');
    const order = options ? options.order : undefined;
    if (order !== undefined && order !== 'hits') throw new TypeError("traceRays: order is 'hits' or left out");
    const volume = options ? options.volume : undefined;
    if (volume !== undefined && (!volume || !volume._handle)) throw new TypeError('traceRays: volume is what bakeVolume returned');
    const gain = options && options.gain !== undefined ? options.gain : Math.fround(1 / Math.PI);
    if (volume !== undefined && typeof gain !== 'number') throw new TypeError('traceRays: gain is a number');
    this._uploadFrameState();
    return traceRaysOn(this._context(), rays, this.traceParams(options), order === 'hits' ? 1 : 0, volume ? volume._handle : undefined, gain);
  }

  /* LIGHT PROBES: probe positions in, one spherical-harmonic row per probe out, the rays and their radiance never leaving the device (flx_probes_sh,
   * include/flexlight_hip_debug.h "light probes").  positions: Float32Array, 3 or 4 floats per probe (options.stride names which; by default 4 where the length is a
   * multiple of 4 and not of 3, else 3).  options: traceRays' (order included) plus faceSize (1 .. 256, by default 8: 6 x 8 x 8 rays a probe) and sky ([r, g, b], the
   * radiance of a ray that hits nothing, by default 0 0 0).  Returns a Float32Array of 36 floats per probe: coefficient i (real SH bands 0 - 2), channel c in word
   * 4 i + c; words 3, 7, 11, 15 the sums of d_omega, of d_omega over the rays that hit, of d_omega s and of d_omega s s over them.  It waits for the answer. */
  traceProbes (positions, options) {
    if (this._devices) throw new Error('traceProbes: one GPU only (a group of GPUs traces no rays)');
    if (!(positions instanceof Float32Array)) throw new TypeError('traceProbes: positions is a Float32Array of 3 or 4 floats per probe');
    const o = options || {};
    if (o.order !== undefined && o.order !== 'hits') throw new TypeError("traceProbes: order is 'hits' or left out");
    const stride = o.stride !== undefined ? o.stride : (positions.length % 4 === 0 && positions.length % 3 !== 0 ? 4 : 3);
    if ((stride !== 3 && stride !== 4) || positions.length % stride !== 0) throw new TypeError('traceProbes: positions is a Float32Array of 3 or 4 floats per probe');
    let rows = positions;
    if (stride === 3) {
      rows = new Float32Array(positions.length / 3 * 4);
      for (let k = 0; k < positions.length / 3; k++) { rows[4 * k] = positions[3 * k]; rows[4 * k + 1] = positions[3 * k + 1]; rows[4 * k + 2] = positions[3 * k + 2]; }
    }
    const sky = o.sky === undefined ? [0, 0, 0] : Array.from(o.sky);
    if (sky.length !== 3) throw new TypeError('traceProbes: sky is [r, g, b]');
    this._uploadFrameState();
    const probe = { faceSize: o.faceSize === undefined ? 8 : o.faceSize, order: o.order === 'hits' ? 1 : 0, sky };
    return new Float32Array(native().traceProbes(this._context(), rows, this.traceParams(options), probe));
  }

  /* The irradiance an SH row of traceProbes gives for a normal (flx_probe_irradiance, the definition Python shares): row Float32Array(36) — a probe's part of
   * traceProbes' result, row.subarray(36 k, 36 k + 36) —, normal [x, y, z], used as given.  Returns Float32Array(3).  Needs no GPU call. */
  probeIrradiance (row, normal) {
    if (this._devices) throw new Error('probeIrradiance: one GPU only (a group of GPUs traces no rays)');
    if (!(row instanceof Float32Array) || row.length !== 36) throw new TypeError('probeIrradiance: row is a Float32Array of 36 floats');
    return native().probeIrradiance(row.byteOffset === 0 && row.buffer.byteLength === 144 ? row : Float32Array.from(row), Float32Array.from(normal));
  }

  /* PROBE VOLUMES: a regular grid of light probes baked on the device, and the irradiance it gives surface points (include/flexlight_hip_debug.h "probe volumes").
   * grid: { origin: [x, y, z], spacing: [x, y, z], count: [nx, ny, nz], normalBias = 0, floor = 0.05, visibility = true } — probe (ix, iy, iz) lies at
   * origin + i * spacing and has index (iz ny + iy) nx + ix.  options: traceProbes' (faceSize, sky, order and traceRays').  Returns a handle { grid, probes,
   * rows() } whose SH rows STAY ON THE DEVICE (flx_volume_bake_device): renderIrradiance and irradianceRays read them there; rows() fetches them as a Float32Array of
   * 36 floats per probe, traceProbes' rows of the grid's positions bit for bit.  It waits for the bake.
   * options.map = { size: 1 .. 16, sharpness: 0 .. 8 = 5 }: DIRECTIONAL VISIBILITY ("directional visibility", flx_volume_bake_map_device) — every probe also gets an
   * octahedral map of size x size bins of distance moments, baked from the same rays and kept on the device beside the SH rows; renderIrradiance and
   * irradianceRays then weigh a probe by what it sees TOWARDS the point, not all around: walls stop leaking and open rooms are not dimmed.  The handle has map and
   * maps() (4 floats per bin) then.  Without options.map every call does what it did.
   * options.relocate = relocateVolume's options: PROBE RELOCATION first, from zero offsets, and the bake from the moved positions (flx_volume_bake_relocated_device);
   * the handle has offsets() and states() then, and every later call on it goes through the relocated calls. */
  bakeVolume (grid, options) {
    if (this._devices) throw new Error('bakeVolume: one GPU only (a group of GPUs traces no rays)');
    const o = options || {};
    if (o.order !== undefined && o.order !== 'hits') throw new TypeError("bakeVolume: order is 'hits' or left out");
    const three = (v, what) => { const a = Array.from(v || []); if (a.length !== 3) throw new TypeError('bakeVolume: ' + what + ' is [x, y, z]'); return a; };
    const g = { origin: three(grid.origin, 'origin'), spacing: three(grid.spacing, 'spacing'), count: three(grid.count, 'count'),
      normalBias: grid.normalBias === undefined ? 0 : grid.normalBias, floor: grid.floor === undefined ? 0.05 : grid.floor, visibility: grid.visibility === undefined ? true : !!grid.visibility };
    const sky = o.sky === undefined ? [0, 0, 0] : Array.from(o.sky);
    if (sky.length !== 3) throw new TypeError('bakeVolume: sky is [r, g, b]');
    this._uploadFrameState();
    const context = this._context();
    const probe = { faceSize: o.faceSize === undefined ? 8 : o.faceSize, order: o.order === 'hits' ? 1 : 0, sky };
    if (o.map !== undefined) {
      if (o.map === null || typeof o.map !== 'object' || typeof o.map.size !== 'number') throw new TypeError('bakeVolume: map is { size, sharpness }');
      probe.map = { size: o.map.size, sharpness: o.map.sharpness === undefined ? 5 : o.map.sharpness };
    }
    if (o.relocate !== undefined) probe.relocate = this._relocateOptions(o.relocate, 'bakeVolume');
    const handle = native().bakeVolume(context, g, this.traceParams(options), probe);
    const volume = { grid: g, probes: g.count[0] * g.count[1] * g.count[2], _handle: handle, rows: () => new Float32Array(native().volumeRows(context, handle)) };
    if (probe.map) Object.assign(volume, { map: probe.map, maps: () => new Float32Array(native().volumeMaps(context, handle)) });
    if (probe.relocate) this._withOffsets(volume, context);
    return volume;
  }

  /* relocateVolume's options with their defaults -> what the addon reads; `call`: the method's name, for the messages */
  _relocateOptions (options, call) {
    const o = options || {};
    if (o === null || typeof o !== 'object') throw new TypeError(call + ': relocate is { backShare, minFront, reach, limit, iterations, faceSize }');
    for (const k of ['minFront', 'reach']) if (typeof o[k] !== 'number') throw new TypeError(call + ': ' + k + ' is a number (world units)');
    const r = { backShare: o.backShare === undefined ? 0.25 : o.backShare, minFront: o.minFront, reach: o.reach, limit: o.limit === undefined ? 0.45 : o.limit,
      iterations: o.iterations === undefined ? 4 : o.iterations, faceSize: o.faceSize === undefined ? 8 : o.faceSize };
    if (!Number.isInteger(r.iterations) || r.iterations < 0 || r.iterations > 64) throw new RangeError(call + ': iterations is a whole number, 0 .. 64');
    if (!Number.isInteger(r.faceSize) || r.faceSize < 0 || r.faceSize > 0xffffffff) throw new RangeError(call + ': faceSize is a whole number');
    return r;
  }

  /* a handle that has offsets: offsets() fetches them (4 floats per probe: x, y, z and the state's bits), states() the state words */
  _withOffsets (volume, context) {
    const handle = volume._handle;
    volume.offsets = () => new Float32Array(native().volumeOffsets(context, handle));
    volume.states = () => Uint32Array.from(new Uint32Array(native().volumeOffsets(context, handle)).filter((_, i) => i % 4 === 3));
    return volume;
  }

  /* PROBE RELOCATION (include/flexlight_hip_debug.h "probe relocation", flx_volume_relocate_device): probes that lie inside geometry or within a hair of a wall are
   * moved — out of geometry, away from a near wall, back towards the lattice where there is room — and probes that are inside something or see no front face
   * within reach are switched off.  options: { backShare = 0.25, minFront, reach, limit = 0.45, iterations = 4, faceSize = 8 }; minFront and reach are world units.
   * The handle keeps an offsets array on the device, zero-filled at the first call; `iterations` passes run and then one frozen pass, which moves nothing and
   * classifies every probe where it stands.  Returns { offsets: Float32Array (4 floats per probe: x, y, z and the state's bits), states: Uint32Array (bit 0
   * inactive, bits 1 - 2 the rule that fired, bit 3 rejected) }.  From then on updateVolume, renderIrradiance and irradianceRays on this handle take the relocated
   * calls: a probe stands at its lattice point plus its offset, and an inactive probe gets no weight.  The handle's rows and maps are NOT re-baked: call
   * updateVolume with hysteresis 0 over the probes that moved, or bake with bakeVolume(grid, { relocate }) in the first place.  It waits for the passes. */
  relocateVolume (volume, options) {
    if (this._devices) throw new Error('relocateVolume: one GPU only (a group of GPUs casts no rays)');
    if (!volume || !volume._handle) throw new TypeError('relocateVolume: volume is what bakeVolume returned');
    const r = this._relocateOptions(options, 'relocateVolume');
    this._uploadFrameState();
    const context = this._context();
    const buffer = native().relocateVolume(context, volume._handle, Math.floor(2048 / this.scene.standardTextureSizes[0]), r);
    if (!volume.offsets) this._withOffsets(volume, context);
    return { offsets: new Float32Array(buffer), states: Uint32Array.from(new Uint32Array(buffer).filter((_, i) => i % 4 === 3)) };
  }

  /* VOLUME UPDATES (include/flexlight_hip_debug.h "volume updates", flx_volume_update_device): a baked volume kept alive over many frames.  The probes named by
   * options.probes — a Uint32Array of indices, or { first, stride, count } for probe first + j * stride (a rotating subset is first = frame % stride) — are traced
   * again with the face size, sky and order the volume was baked with and with options' traceRays' fields (vary randomSeed from update to update), and the new rows
   * are blended into the handle's resident rows, and its maps if it has them, IN PLACE on the device: old + (new - old) (1 - options.hysteresis).  A new row that
   * holds a NaN or an infinity is rejected; a probe that was never baked takes the new row.  Returns { states: Uint32Array }, per entry 0 blended, 1 taken, 2 kept,
   * 3 skipped (an index outside the grid).  It waits for the update.  A list that names a probe twice gives that probe one of the possible results.
   * A handle that has offsets (relocateVolume) traces the listed probes from their offset positions (flx_volume_update_relocated_device). */
  updateVolume (volume, options) {
    if (this._devices) throw new Error('updateVolume: one GPU only (a group of GPUs traces no rays)');
    if (!volume || !volume._handle) throw new TypeError('updateVolume: volume is what bakeVolume returned');
    const o = options || {};
    if (typeof o.hysteresis !== 'number') throw new TypeError('updateVolume: hysteresis is a number');
    const list = { hysteresis: o.hysteresis };
    if (o.probes instanceof Uint32Array) list.indices = o.probes.byteOffset === 0 && o.probes.buffer.byteLength === o.probes.byteLength ? o.probes : Uint32Array.from(o.probes);
    else if (o.probes !== null && typeof o.probes === 'object' && ['first', 'stride', 'count'].every(k => Number.isInteger(o.probes[k]) && o.probes[k] >= 0 && o.probes[k] <= 0xffffffff)) {
      Object.assign(list, { first: o.probes.first, stride: o.probes.stride, count: o.probes.count });
    } else throw new TypeError('updateVolume: probes is a Uint32Array of indices or { first, stride, count }');
    this._uploadFrameState();
    return { states: new Uint32Array(native().updateVolume(this._context(), volume._handle, this.traceParams(options), list)) };
  }

  /* The irradiance IMAGE of the frame the next renderFrame() would trace without jitter (flx_frame_irradiance_device; flx_frame_irradiance_map_device where the
   * volume was baked with a map): per pixel the irradiance the volume gives
   * the primary hit's position and ray-facing normal — r g b and the sum of the weights; a pixel that hits nothing is 0 0 0 0.  Nothing but the image crosses the
   * bus.  volume: bakeVolume's handle; one that has offsets (relocateVolume) goes through flx_frame_irradiance_relocated_device, as irradianceRays goes through
   * flx_rays_irradiance_relocated_device.  Returns a Float32Array of 4 floats per pixel, row 0 on top, with width and height beside it. */
  renderIrradiance (volume) {
    if (this._devices) throw new Error('renderIrradiance: one GPU only (a group of GPUs casts no rays)');
    if (!volume || !volume._handle) throw new TypeError('renderIrradiance: volume is what bakeVolume returned');
    this._uploadFrameState();
    const p = this.frameParams();
    return Object.assign(new Float32Array(native().frameIrradiance(this._context(), p, volume._handle)), { width: p.width, height: p.height });
  }

  /* The same for rays of the application's own (flx_rays_irradiance_device; flx_rays_irradiance_map_device where the volume was baked with a map): rays are castRays' rows; returns a Float32Array of 4 floats per ray. */
  irradianceRays (rays, volume) {
    if (this._devices) throw new Error('irradianceRays: one GPU only (a group of GPUs casts no rays)');
    if (!(rays instanceof Float32Array) || rays.length % 8 !== 0) throw new TypeError('irradianceRays: rays is a Float32Array of 8 floats per ray');
    if (!volume || !volume._handle) throw new TypeError('irradianceRays: volume is what bakeVolume returned');
    this._uploadFrameState();
    return new Float32Array(native().raysIrradiance(this._context(), rays, Math.floor(2048 / this.scene.standardTextureSizes[0]), volume._handle));
  }

  /* A ray IMAGE, traced and DENOISED: any projection the application makes rays for — a panorama, a fisheye or orthographic view, a stereo pair, a probe's faces, a
   * reflection buffer — through the renderer's own filter (flx_rays_image, include/flexlight_hip_debug.h "ray queries").  rays: traceRays' rows, width * height of
   * them in image order, row 0 on top.  options: traceRays' plus hdr (by default config.hdr), the chain's tone map.  Per ray the five filter planes are what a frame
   * with config.filter writes for a pixel (the samples run in order on one state; a miss is zeros), and the chain over them is the frame's.  Returns { width,
   * height, radiance: Float32Array(4 n) }.  It waits for the answer; frames in flight finish unchanged.
   * FROM A CAMERA: rays may be a camera description instead (cameraOf: { projection: 'panorama', position, basis, extent, jitter, face }; {} is the engine's own
   * pinhole camera): the rays are made on the device (flx_camera_image) and NOTHING BUT THE IMAGE crosses the bus.  The image is, byte for byte, that of
   * traceImage(cameraRays(description, width, height), width, height, options); options.temporal works the same way.
   * OVER TIME: with options.temporal the image is accumulated over one of the context's 8 ray-image histories (flx_rays_image_temporal), as a frame is with
   * config.temporal: options { temporal: true, history = 0, temporalSamples = config.temporalSamples, filter = true, randomSeed }.  The same width * height rays in
   * the same order are traced again call after call; a ray whose first hit moved starts over.  The renderer keeps a frame counter per history and passes
   * counter % N as the seed (N: temporalSamples, 4 where it is <= 0, at most 16) unless randomSeed is given; the counter restarts with resetRayHistory(history) and
   * with a change of size or N, as the history does.  Without the filter the temporal pass' colour is returned.
   * WITH A VOLUME: options.volume, bakeVolume's handle, and options.gain — by default Math.fround(1 / Math.PI) — are traceRays' (flx_rays_image_gather and its
   * kin, "ray images with a volume"): every sample of every ray ends in the volume's irradiance at its last surface point times the gain where it ends in
   * scene.ambientLight without, the lookup inline in the planes kernel; one or two bounces, the volume, the denoiser and the temporal pass are what an application
   * puts on screen.  It works in all four forms — rays or a camera, with and without temporal; the histories are the same eight, and a history does not know
   * whether a volume lit it: resetRayHistory is the caller's business.  A volume that is no handle and a gain that is no number are TypeErrors.  Without
   * options.volume the call is what it was. */
  traceImage (rays, width, height, options) {
    if (this._devices) throw new Error('traceImage: one GPU only (a group of GPUs traces no rays)');
    const volume = options ? options.volume : undefined;
    if (volume !== undefined && (!volume || !volume._handle)) throw new TypeError('traceImage: volume is what bakeVolume returned');
    const gain = options && options.gain !== undefined ? options.gain : Math.fround(1 / Math.PI);
    if (volume !== undefined && typeof gain !== 'number') throw new TypeError('traceImage: gain is a number');
    const camera = isCameraDescription(rays) ? this.cameraOf(rays, width, height, 'traceImage') : null;      // the rays are made on the device: none cross the bus
    if (!camera) {
      if (!(rays instanceof Float32Array) || rays.length % 8 !== 0) throw new TypeError('traceImage: rays is a Float32Array of 8 floats per ray, or a camera description');
      if (!Number.isInteger(width) || !Number.isInteger(height) || width < 0 || height < 0 || rays.length / 8 !== width * height) {
        throw new RangeError('traceImage: rays is width * height rays in image order');
      }
    }
    this._uploadFrameState();
    const hdr = options && options.hdr !== undefined ? !!options.hdr : !!this.config.hdr;
    if (options && options.temporal) {
      const history = options.history === undefined ? 0 : options.history;
      if (!Number.isInteger(history) || history < 0 || history > 7) throw new RangeError('traceImage: history is one of 0 .. 7');
      const temporalSamples = options.temporalSamples === undefined ? this.config.temporalSamples : options.temporalSamples;
      const depth = temporalSamples <= 0 ? 4 : Math.min(16, temporalSamples);      // flx_frame_params' rule
      if (!this._rayHistories) this._rayHistories = {};
      let h = this._rayHistories[history];
      if (!h || h.width !== width || h.height !== height || h.depth !== depth) h = this._rayHistories[history] = { width, height, depth, counter: 0 };
      const params = this.traceParams(options);
      if (options.randomSeed === undefined) params.randomSeed = h.counter % depth;
      const filter = options.filter === undefined ? true : !!options.filter;
      const over = { history, temporalSamples, filter, hdr };
      const image = volume
        ? (camera ? native().cameraImageTemporalGather(this._context(), camera, width, height, params, over, volume._handle, gain)
          : native().rayImageTemporalGather(this._context(), rays, width, height, params, over, volume._handle, gain))
        : camera ? native().cameraImageTemporal(this._context(), camera, width, height, params, over) : native().rayImageTemporal(this._context(), rays, width, height, params, over);
      h.counter++;
      return { width, height, radiance: new Float32Array(image) };
    }
    const image = volume
      ? (camera ? native().cameraImageGather(this._context(), camera, width, height, this.traceParams(options), hdr, volume._handle, gain)
        : native().rayImageGather(this._context(), rays, width, height, this.traceParams(options), hdr, volume._handle, gain))
      : camera ? native().cameraImage(this._context(), camera, width, height, this.traceParams(options), hdr) : native().rayImage(this._context(), rays, width, height, this.traceParams(options), hdr);
    return { width, height, radiance: new Float32Array(image) };
  }

  /* The rays of a camera, made on the device (flx_camera_rays, include/flexlight_hip_debug.h "cameras"): traceRays' rows, w * h of them in image order, row 0 on
   * top, whose noise words are the pixels' positions as a frame has them.  camera: a description (cameraOf); region: [x0, y0, w, h] of the image, by default all
   * of it — a region's rows are the whole image's rows of those pixels.  Needs no scene.  Returns a Float32Array of 8 floats per ray: what castRays, traceRays,
   * surfaceRays and traceImage take.  (traceImage takes the description itself: then no rays come back to the host at all.) */
  cameraRays (camera, width, height, region) {
    if (this._devices) throw new Error('cameraRays: one GPU only (a group of GPUs traces no rays)');
    if (!isCameraDescription(camera)) throw new TypeError('cameraRays: camera is a camera description');
    if (region !== undefined && region !== null && !(Array.isArray(region) && region.length === 4)) throw new TypeError('cameraRays: region is [x0, y0, w, h]');
    return new Float32Array(native().cameraRays(this._context(), this.cameraOf(camera, width, height, 'cameraRays'), width, height, region || null));
  }

  /* A camera description -> the library's flx_camera.  { projection, position, basis, extent, jitter, face }, all optional:
   *   projection  'pinhole' (the default) | 'panorama' | 'fisheye' | 'orthographic' | 'cubeFace'
   *   position    [x, y, z], by default the engine's camera's
   *   basis       9 numbers.  The pinhole: a frame's view matrix, BY DEFAULT sceneFile.buildViewMatrix(this.camera, width, height) — {} is the engine's own camera, and
   *               its image is the frame's.  The others: rows right, up, forward in world space, used as given; by default the identity.
   *   extent      panorama: [horizontal, vertical] angle in radians (by default the sphere, [2 pi, pi]); fisheye: [field of view across the width] (by default pi);
   *               orthographic: [width, height] of the window in world units (by default [1, 1])
   *   jitter      [x, y] sub-pixel offset in pixels, each in [-0.5, 0.5]; by default none
   *   face        cubeFace: 0 .. 5 = +x -x +y -y +z -z */
  cameraOf (description, width, height, call) {
    const d = description, who = call || 'cameraOf';
    const projection = d.projection === undefined ? 'pinhole' : d.projection;
    const code = CAMERA_PROJECTIONS.indexOf(projection);
    if (code < 0) throw new RangeError(who + ': projection is one of ' + CAMERA_PROJECTIONS.join(', '));
    const numbers = (v, n, name) => {
      const a = Array.from(v);
      if (a.length !== n || a.some(x => typeof x !== 'number')) throw new TypeError(who + ': ' + name + ' is ' + n + ' numbers');
      return a;
    };
    const defaults = [[0, 0], [2 * Math.PI, Math.PI], [Math.PI, 0], [1, 1], [0, 0]][code];
    const extent = d.extent === undefined ? defaults : Array.from(d.extent).concat(defaults.slice(Array.from(d.extent).length));
    return {
      projection: code,
      face: d.face === undefined ? 0 : d.face,
      position: d.position === undefined ? [this.camera.x, this.camera.y, this.camera.z] : numbers(d.position, 3, 'position'),
      basis: d.basis !== undefined ? numbers(d.basis, 9, 'basis') : code === 0 ? Array.from(sceneFile.buildViewMatrix(this.camera, width, height)) : [1, 0, 0, 0, 1, 0, 0, 0, 1],
      extent: numbers(extent, 2, 'extent'),
      jitter: d.jitter === undefined ? [0, 0] : numbers(d.jitter, 2, 'jitter')
    };
  }

  /* A ray-image history of traceImage's (by default all of them) starts afresh with the next image: its frame counter and, where a context is up, the library's
   * history (flx_rays_history_reset). */
  resetRayHistory (history) {
    const which = history === undefined ? -1 : history;
    if (!Number.isInteger(which) || which < -1 || which > 7) throw new RangeError('resetRayHistory: history is one of 0 .. 7, or -1 for all');
    if (this._rayHistories) {
      if (which === -1) this._rayHistories = {};
      else delete this._rayHistories[which];
    }
    if (this._ctx) native().rayHistoryReset(this._ctx, which);
  }

  /* What the SURFACE is where rays of the application's own first hit: the inputs of a denoiser, of compositing, of a hybrid renderer's shading
   * (flx_rays_surface, include/flexlight_hip_debug.h "surface rows").  rays: castRays' rows (words 3 and 7 are ignored); fields: SURFACE bits (by default all).
   * Returns typed arrays per plane asked for, 4 floats a ray — hit (s, u, v, -), position (x y z, 1 for a hit), geometryNormal, normal (facing the ray; w: -1
   * front face, +1 back face), uv (u, v, -, 0), albedo, rme, tpo —, entry: Int32Array(n) with hit, transform: Int32Array(n) with uv.  A miss is all zeros,
   * entry -1.  It waits for the answer; frames in flight finish unchanged. */
  surfaceRays (rays, fields) {
    if (this._devices) throw new Error('surfaceRays: one GPU only (a group of GPUs casts no rays)');
    this._uploadFrameState();
    return surfaceRaysOn(this._context(), rays, fields, Math.floor(2048 / this.scene.standardTextureSizes[0]));
  }

  /* The same planes for every pixel of the frame the next renderFrame() would trace without jitter (flx_frame_surface): row k of a plane is pixel k of that frame,
   * the primary hit found as the frame finds it.  Also returns width and height. */
  renderSurface (fields) {
    if (this._devices) throw new Error('renderSurface: one GPU only (a group of GPUs casts no rays)');
    this._uploadFrameState();
    const p = this.frameParams();
    const f = fields === undefined ? SURFACE.ALL : fields;
    return Object.assign(unpackSurface(native().frameSurface(this._context(), p, f), p.width * p.height, f), { width: p.width, height: p.height });
  }

  traceParams (options) {
    const o = options || {};
    const pick = (v, d) => (v === undefined ? d : v);
    return {
      samples: pick(o.samples, this.config.samplesPerRay),
      maxReflections: pick(o.maxReflections, this.config.maxReflections),
      minImportancy: pick(o.minImportancy, this.config.minImportancy),
      ambient: Array.from(pick(o.ambient, this.scene.ambientLight)).slice(0, 3),
      randomSeed: pick(o.randomSeed, 0),
      textureWidth: pick(o.textureWidth, Math.floor(2048 / this.scene.standardTextureSizes[0]))
    };
  }

  renderFrame (options) {
    const gpu = this._uploadFrameState();
    const aa = this._antialiasing();
    const jitter = aa === 'taa' ? this._jitter() : { x: 0, y: 0 };
    const p = this.frameParams(jitter);
    const rows = gpu.rows(p);
    /* options.reuse: write into the array of the frame before (a frame loop that consumes each frame before asking for the
     * next saves a 33 MB allocation per 1080p frame); by default every frame gets its own */
    const n = rows * p.width * 4;
    let radiance = (options && options.reuse && this._out && this._out.length === n) ? this._out : new Float32Array(n);
    this._out = radiance;
    let info;
    if (this._devices && this.config.temporal) {
      /* a temporal frame on a group of GPUs runs in the library's frame loop, where every GPU keeps the history of its own strips (flx_group_render
       * is stateless and refuses it): the frames the loop has in flight are taken first, then this one is begun and taken */
      if (options && options.counters) throw new Error('renderFrame: temporal frames on a group of GPUs are not counted');
      const n = native(), g = this._group;
      while (n.groupFramesInFlight(g) > 0) n.groupFrameEnd(g, this.present8);
      n.groupFrameBegin(g, p, this._tileRows, false);
      const r = n.groupFrameEnd(g, false);
      radiance.set(r.pixels);
      info = { frameMs: r.gpuMs };
    } else info = gpu.render(p, radiance, !!(options && options.counters));
    if (aa && rows === p.height) {                        // the pass reads neighbouring texels: whole frames only (pathtracerWGL2.js:552-553)
      if (this._devices) throw new Error('antialiasing passes run on one context: use a single device');
      const out = new Float32Array(radiance.length);
      if (aa === 'fxaa') native().fxaa(this._context(), p.width, p.height, radiance, out);
      else native().taa(this._context(), p.width, p.height, radiance, out);
      radiance = out;
    }
    this._temporalFrame = (this._temporalFrame + 1) % Math.max(1, this.config.temporalSamples);     // pathtracerWGL2.js:291
    this.lastFrame = Object.assign({ width: p.width, height: p.height, rows, radiance }, info);
    return this.lastFrame;
  }

  /* The RGBA8 the reference's canvas would hold for a frame of renderFrame() (whole frames): { width, height, data: Uint8ClampedArray },
   * the shape of an ImageData. */
  presentFrame (frame) {
    const f = frame || this.lastFrame;
    if (!f || f.rows !== f.height) throw new Error('presentFrame: a whole frame of renderFrame() is needed');
    const data = new Uint8ClampedArray(f.width * f.height * 4);
    native().present(this._context(), f.width, f.height, f.radiance, data);
    return { width: f.width, height: f.height, data };
  }

  /* Several frames of a camera path in ONE pass of the GPU pipeline (flx_render_batch; not in the reference, which renders frame
   * after frame): `cameras` is an array of up to 32 camera states { x, y, z, fx, fy } (missing fields default to this.camera's;
   * fov comes from this.camera).  Frames without temporal accumulation and anti-aliasing only — those depend on the frames
   * before (filter frames are fine: their chain starts from the same state every frame).  Returns { width, height, rows, frames: [Float32Array(rows*width*4), ...], frameMs, counters? }; every frame equals
   * the renderFrame() of its camera. */
  renderBatch (cameras, options) {
    if (this.config.temporal || this._antialiasing()) throw new Error('renderBatch: temporal and antialiasing frames depend on the frames before');
    const gpu = this._uploadFrameState();
    const saved = this.camera;
    const params = cameras.map(c => {
      this.camera = Object.assign(Object.create(saved), c);
      try { return this.frameParams(); } finally { this.camera = saved; }
    });
    const rows = gpu.rows(params[0]);
    const per = rows * params[0].width * 4;
    const all = new Float32Array(per * params.length);
    const info = gpu.renderBatch(params, all, !!(options && options.counters));
    const frames = params.map((_, i) => all.subarray(i * per, (i + 1) * per));
    return Object.assign({ width: params[0].width, height: params[0].height, rows, frames }, info);
  }

  /* The frame loop (pathtracerWGL2.js:191-831).  Like the reference's, it does not wait for the GPU inside a frame: frame
   * k + 1 is prepared and enqueued (flx_frame_begin) while frame k is traced and copied to pinned host memory, then frame k is
   * taken (flx_frame_end) and handed to canvas.onFrame — `pixels` is a view of that pinned memory (Float32Array, or the canvas'
   * RGBA8 as a Uint8ClampedArray with this.present8), valid until the frame after the next is begun.  A group of GPUs (`devices`) runs the
   * same loop through flx_group_frame_begin / _end with up to this.groupLanes (3) frames in flight, `pixels` valid until the next frame is begun.
   * One context runs the anti-aliasing pass inside the library's loop too (frameBegin's { antialiasing }: FLX_FRAME_FXAA / FLX_FRAME_TAA, the TAA
   * jitter drawn per frame as renderFrame() draws it); tiles, and a group with a pass, take the synchronous renderFrame() per cycle instead.  `fps` as in pathtracerWGL2.js:293-298;
   * `gpuMs` = GPU time of the last frame taken. */
  async render () {
    if (!this._halt) return;                              // already running (the WebGPU renderer guards the same way)
    this._halt = false;
    await this.updateScene();
    let frames = 0, windowStart = Date.now();
    this._inFlight = 0;
    const pending = [];                                    // sizes of the frames begun and not yet taken
    const deliver = frame => {
      this.lastFrame = frame;
      if (typeof this._canvas.onFrame === 'function') this._canvas.onFrame(frame);
      frames++;
      const now = Date.now();
      if (now - windowStart >= 500) {                     // pathtracerWGL2.js:293-298
        this.fps = (1000 * frames / (now - windowStart)).toFixed(0);
        frames = 0; windowStart = now;
      }
    };
    /* flx_frame_end waits for the GPU: on a worker thread (frameEndAsync: napi_async_work), so that this thread is back in the event loop for most of every frame,
     * as the reference's is (pathtracerWGL2.js:300-302).  this.blockingFrameEnd = true: the synchronous call, for measurements. */
    const take = async () => {
      const q = pending.shift();
      let r;
      if (this.blockingFrameEnd) r = q.group ? native().groupFrameEnd(this._group, q.rgba8) : native().frameEnd(this._ctx, q.rgba8);
      else {
        this._pendingEnd = q.group ? native().groupFrameEndAsync(this._group, q.rgba8) : native().frameEndAsync(this._ctx, q.rgba8);
        try { r = await this._pendingEnd; } finally { this._pendingEnd = null; }
      }
      this._inFlight--;
      if (this._releaseWhenIdle) {                          // halt() came while the frame was being waited for: its memory goes now
        this._releaseWhenIdle = false;
        this._release();
        return;
      }
      this.gpuMs = r.gpuMs;
      deliver({ width: q.width, height: q.height, rows: q.rows, radiance: q.rgba8 ? undefined : r.pixels, rgba8: q.rgba8 ? r.pixels : undefined, pixels: r.pixels, frameMs: r.gpuMs });
    };
    const cycle = async () => {
      if (this._halt) return;
      try {
        const aa = this._antialiasing();
        /* a group of GPUs (flx_group_frame_begin / _end): every GPU's frame server resolves its strips straight into one image in pinned host memory, up to
         * three frames in flight, nothing waits for a GPU inside a frame; `pixels` is a view of that image, the frame's until the next frame is begun */
        const grouped = !!this._devices && !this._tile && !aa;      // (present8: the servers quantise their tiles as they resolve them — the canvas' bytes, a quarter of what every GPU writes)
        const pipelined = !this._devices && !this._tile;
        if (grouped) {
          this._uploadFrameState();
          const p = this.frameParams();
          if (this._lanesSet !== this.groupLanes) {         // (the library's default is 3)
            while (this._inFlight > 0 && !this._halt) await take();
            if (this._halt) return;
            native().groupSetFrameLanes(this._group, this.groupLanes);
            this._lanesSet = this.groupLanes;
          }
          if (this._inFlight === this.groupLanes) await take();
          if (this._halt) return;                           // (the application halted the renderer from its onFrame)
          native().groupFrameBegin(this._group, p, this._tileRows, this.present8);
          this._inFlight++;
          pending.push({ width: p.width, height: p.height, rows: p.height, rgba8: this.present8, group: true });
          this._temporalFrame = (this._temporalFrame + 1) % Math.max(1, this.config.temporalSamples);
        } else if (pipelined) {
          this._uploadFrameState();
          const p = aa ? this.frameParams(aa === 'taa' ? this._jitter() : { x: 0, y: 0 }) : this.frameParams();      // (the camera renderFrame() gives the pass)
          if (aa) native().frameBegin(this._context(), p, this.present8, { antialiasing: aa });
          else native().frameBegin(this._context(), p, this.present8);
          this._inFlight++;
          pending.push({ width: p.width, height: p.height, rows: p.height, rgba8: this.present8 });
          this._temporalFrame = (this._temporalFrame + 1) % Math.max(1, this.config.temporalSamples);
          if (this._inFlight === 2) await take();
        } else {
          while (this._inFlight > 0 && !this._halt) await take();
          if (this._halt) return;
          deliver(this.renderFrame({ reuse: true }));
        }
      } catch (e) {
        console.error(e);
        this._halt = true;
        return;
      }
      if (this._halt) return;
      if (this.fpsLimit === Infinity) setImmediate(cycle);
      else setTimeout(cycle, 1000 / this.fpsLimit);
    };
    setImmediate(cycle);
  }
}

/* taa.js:130-149: n two-dimensional offsets that add up to zero */
function taaVectors (n, random) {
  const vecs = new Array(n).fill(0).map(() => new Array(2));
  vecs[0] = [0, 1];
  vecs[1] = [1, 0];
  const combined = [1, 1];
  for (let i = 2; i < n; i++) {
    for (let j = 0; j < 2; j++) {
      const lo = Math.max(-Math.min(i + 1, n - 1 - i), combined[j] - 1);
      const hi = Math.min(Math.min(i + 1, n - 1 - i), combined[j] + 1);
      vecs[i][j] = 0.5 * ((hi + lo) + (hi - lo) * Math.sign(random() - 0.5) * Math.pow(random() * 0.5, 1 / 2)) - combined[j];
      combined[j] += vecs[i][j];
    }
  }
  return vecs;
}

module.exports = { PathTracerHIP, taaVectors, native, castRaysOn, surfaceRaysOn, SURFACE };
