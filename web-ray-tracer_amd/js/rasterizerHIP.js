'use strict';
/*
 * RasterizerHIP — FlexLight's rasterizer renderer (reference modules/rasterizerWGL2.js) with its frames drawn by
 * libflexlight_hip.so (flx_raster_render, k_raster) instead of by WebGL2.  Same surface as the reference's object:
 * type = 'rasterizer', public config / camera / scene, fps, fpsLimit, canvas getter, async render(), halt(),
 * async updateScene(), async updatePrimaryLightSources() — plus renderFrame(), a synchronous single frame for headless use,
 * and presentFrame() as PathTracerHIP has them.  One GPU context (no groups of GPUs).  render() runs the library's frame loop
 * (flx_frame_begin with FLX_FRAME_RASTERIZER) and takes every frame with the blocking frameEnd: no native work is ever pending
 * between ticks, and updateScene() / updatePrimaryLightSources() may run at any time.
 * The "canvas" is any object with width and height; if it has onFrame(frame) the loop calls it.
 */
const { Transform } = require('./scene.js');
const sceneFile = require('./sceneFile.js');
const { native, taaVectors, castRaysOn, surfaceRaysOn } = require('./pathtracerHIP.js');

class RasterizerHIP {
  constructor (canvas, scene, camera, config, options) {
    this.type = 'rasterizer';
    this.config = config;
    this.camera = camera;
    this.scene = scene;
    this.fps = 0;
    this.fpsLimit = Infinity;
    this._canvas = canvas;
    this._device = (options && options.device) || 0;
    this._tile = (options && options.tile) || null;      // {rows, index, count}: this context's strips of the frame
    this.present8 = !!(options && options.present8);     // the frame loop hands out the canvas' RGBA8 instead of the float frame
    this._ctx = null;
    this._pending = [];                                  // the frame loop's frames begun and not yet taken
    this._halt = true;
    this._atlasLists = [null, null, null];
    this._haveScene = false;
    this.lastFrame = null;
  }

  get canvas () { return this._canvas; }

  _context () {
    if (!this._ctx) this._ctx = native().createContext(this._device);
    return this._ctx;
  }

  halt () {                                               // rasterizerWGL2.js:50-57
    this._halt = true;
    if (this._ctx) {
      try { native().destroyContext(this._ctx); } catch (e) { console.warn('Unable to release the GPU context', e.message); }
      this._ctx = null;
    }
    this._haveScene = false;
    this._built = null;
    this._atlasLists = [null, null, null];
    this._pending = [];                                  // (frames in flight: the library waits for them as the context goes)
  }

  /* rasterizerWGL2.js:150-190; as PathTracerHIP.updateScene(): the changed rows alone where only vertices and attributes moved (flx_scene_update refits the
   * boxes on the device), the whole upload otherwise.  lastSceneUpload: 'full' | 'rows' | 'none'. */
  async updateScene () {
    const built = await this.scene.generateArraysFromGraph();
    const rows = this._haveScene ? sceneFile.changedRows(this._built, built) : null;
    if (!rows) return this._uploadBuilt(built);
    if (rows.count > 0) {
      native().updateSceneRows(this._context(), rows.first, built.geometryBuffer.subarray(rows.first * 12, (rows.first + rows.count) * 12),
        built.sceneBuffer.subarray(rows.first * 28, (rows.first + rows.count) * 28));
    }
    this._built = built;
    this.lastSceneUpload = rows.count > 0 ? 'rows' : 'none';
  }

  _uploadBuilt (built) {
    native().uploadScene(this._context(), built.geometryBuffer, built.sceneBuffer, built.idBuffer);
    this._built = built;                                 // (what the device holds: the next updateScene() compares with it)
    this._haveScene = true;
    this.lastSceneUpload = 'full';
  }

  async updatePrimaryLightSources () {                    // rasterizerWGL2.js:125-148
    native().uploadLights(this._context(), sceneFile.buildLightArray(this.scene));
  }

  _updateAtlases () {                                     // rasterizerWGL2.js:65-123: rebuilt only when the list object or its members changed
    const n = native(), c = this._context();
    if (this.scene.prebuiltAtlases) {
      if (this._atlasLists[0] !== this.scene.prebuiltAtlases) {
        this.scene.prebuiltAtlases.forEach((a, which) => n.uploadAtlas(c, which, a.data, a.width, a.height));
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
      if (list.length === 0) { n.uploadAtlas(c, which, null, 0, 0); return; }
      this._atlasLists[which].cells = [sizes[0], sizes[1]];      // what the resident atlas is built with (uploadTextures: the device resamples and composites, sceneFile.buildAtlas' bytes)
      if (old && old.cells && old.length === list.length && old.cells[0] === sizes[0] && old.cells[1] === sizes[1]) {
        list.forEach((e, i) => { if (e !== old[i]) n.updateTexture(c, which, i, sceneFile.nativeTexture(e)); });      // only the members that changed, each into its cell
      } else {
        n.uploadTextures(c, which, list.map(sceneFile.nativeTexture), sizes[0], sizes[1]);
      }
    });
  }

  /* the uniforms of rasterizingPass (rasterizerWGL2.js:253-284); the path-tracing fields the binding requires are fixed */
  frameParams (jitter) {
    const q = this.config.renderQuality > 0 ? this.config.renderQuality : 1;
    const w = Math.max(1, Math.round(this._canvas.width * q)), h = Math.max(1, Math.round(this._canvas.height * q));
    const cam = jitter ? Object.assign(Object.create(this.camera), { fx: this.camera.fx + jitter.x, fy: this.camera.fy + jitter.y }) : this.camera;
    const p = {
      width: w, height: h,
      camera: [this.camera.x, this.camera.y, this.camera.z],
      viewMatrix: Array.from(sceneFile.buildViewMatrix(cam, w, h)),                 // rasterizerWGL2.js:254-265: jittered direction, same matrix as the path tracer's
      samples: 1, maxReflections: 0, minImportancy: 0,
      hdr: this.config.hdr ? 1 : 0,
      ambient: [this.scene.ambientLight[0], this.scene.ambientLight[1], this.scene.ambientLight[2]],
      textureWidth: Math.floor(2048 / this.scene.standardTextureSizes[0])
    };
    if (this._tile) { p.tileRows = this._tile.rows; p.tileIndex = this._tile.index; p.tileCount = this._tile.count; }
    return p;
  }

  /* config.antialiasing: 'fxaa' | 'taa' | anything else = none (rasterizerWGL2.js:216-232); TAA as in PathTracerHIP */
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

  /* One frame, synchronously: scene once, then lights, transforms and atlases as the reference re-derives them every frame
   * (rasterizerWGL2.js:232, 303-305).  Returns {width, height, rows, radiance: Float32Array(rows*width*4), frameMs, counters?};
   * radiance holds the RGBA8 drawing buffer's bytes as k / 255 (after an anti-aliasing pass: that pass's output). */
  _uploadFrameState () {
    const n = native(), c = this._context();
    if (!this._haveScene) this._uploadBuilt(this.scene.generateArraysFromGraph());
    this._updateAtlases();
    n.uploadLights(c, sceneFile.buildLightArray(this.scene));
    const tr = Transform.buildWGL2Arrays();
    n.uploadTransforms(c, tr[0], tr[1]);
  }

  /* PathTracerHIP.castRays(): the same call on the same context plumbing — which object is under the cursor of a rasterized view.  (This renderer has one
   * context and never a group of GPUs: flexlight.js refuses options.devices for it.) */
  castRays (rays, what) {
    this._uploadFrameState();
    return castRaysOn(this._context(), rays, what);
  }

  /* PathTracerHIP.surfaceRays(): the surface under rays of the application's own — the shading inputs for the reflection rays of a hybrid renderer */
  surfaceRays (rays, fields) {
    this._uploadFrameState();
    return surfaceRaysOn(this._context(), rays, fields, Math.floor(2048 / this.scene.standardTextureSizes[0]));
  }

  renderFrame (options) {
    const n = native(), c = this._context();
    this._uploadFrameState();
    const aa = this._antialiasing();
    const p = this.frameParams(aa === 'taa' ? this._jitter() : null);
    const rows = n.tileRowCount(p);
    let radiance = new Float32Array(rows * p.width * 4);
    const info = n.rasterRender(c, p, radiance, !!(options && options.counters));
    if (aa && rows === p.height) {                        // the pass reads neighbouring texels: whole frames only
      const out = new Float32Array(radiance.length);
      if (aa === 'fxaa') n.fxaa(c, p.width, p.height, radiance, out);
      else n.taa(c, p.width, p.height, radiance, out);
      radiance = out;
    }
    this.lastFrame = Object.assign({ width: p.width, height: p.height, rows, radiance }, info);
    return this.lastFrame;
  }

  /* the RGBA8 the reference's canvas would hold for a whole frame of renderFrame(): { width, height, data: Uint8ClampedArray } */
  presentFrame (frame) {
    const f = frame || this.lastFrame;
    if (!f || f.rows !== f.height) throw new Error('presentFrame: a whole frame of renderFrame() is needed');
    const data = new Uint8ClampedArray(f.width * f.height * 4);
    native().present(this._context(), f.width, f.height, f.radiance, data);
    return { width: f.width, height: f.height, data };
  }

  /* The frame loop (rasterizerWGL2.js:201-251) in the library's loop (flx_frame_begin with FLX_FRAME_RASTERIZER, and FLX_FRAME_FXAA /
   * FLX_FRAME_TAA for config.antialiasing on whole frames): every tick enqueues a frame (frameBegin) and, with two in flight, takes the older one
   * with the blocking frameEnd and hands it to canvas.onFrame as { width, height, rows, radiance | rgba8, pixels, frameMs }.  `pixels` is a view
   * of pinned memory (a Float32Array of the drawing buffer's k / 255, or the canvas' RGBA8 as a Uint8ClampedArray with this.present8), valid
   * until the frame after the next one is begun.  `fps` as in :240-245. */
  async render () {
    if (!this._halt) return;
    this._halt = false;
    await this.updateScene();
    let frames = 0, windowStart = Date.now();
    this._pending = [];
    const take = () => {
      const q = this._pending.shift();
      const r = native().frameEnd(this._ctx, q.rgba8);
      const frame = { width: q.width, height: q.height, rows: q.rows, radiance: q.rgba8 ? undefined : r.pixels, rgba8: q.rgba8 ? r.pixels : undefined,
        pixels: r.pixels, frameMs: r.gpuMs };
      this.lastFrame = frame;
      if (typeof this._canvas.onFrame === 'function') this._canvas.onFrame(frame);
      frames++;
      const now = Date.now();
      if (now - windowStart >= 500) {
        this.fps = (1000 * frames / (now - windowStart)).toFixed(0);
        frames = 0; windowStart = now;
      }
    };
    const cycle = () => {
      if (this._halt) return;
      try {
        this._uploadFrameState();
        const aa = this._antialiasing();
        const p = this.frameParams(aa === 'taa' ? this._jitter() : null);
        const rows = native().tileRowCount(p);
        const opts = { renderer: 'rasterizer' };
        if (aa && rows === p.height) opts.antialiasing = aa;      // the pass reads neighbouring texels: whole frames only
        native().frameBegin(this._ctx, p, this.present8, opts);
        this._pending.push({ width: p.width, height: p.height, rows, rgba8: this.present8 });
        if (this._pending.length === 2) take();
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

module.exports = { RasterizerHIP };
