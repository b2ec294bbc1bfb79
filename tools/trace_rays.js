'use strict';
/*
 * Trace rays of one's own through a BASELINE scene by the whole JavaScript path — FlexLight facade, scene graph, host flattening, N-API addon,
 * libflexlight_hip.so (flx_rays_trace) — and write what renderer.traceRays() returns.
 *   node tools/trace_rays.js <scene | file.flxs[.gz]> --rays rays.f32 --out rows.bin [--config-spp S --config-bounces B --samples S --bounces B --seed X --order hits
 *                            --running N --width W --height H --assets DIR --filter WxH --hdr 0|1 --temporal N --frames F --history H --chain 0|1 --reset K]
 *   <scene>: a BASELINE scene built through the scene graph (scenes/index.js), or a .flxs file replayed (sceneFile.sceneFromFlxs: a box without the assets)
 *   --config-spp, --config-bounces: the renderer's config (by default the scene's BASELINE frame); --samples, --bounces, --seed: traceRays' options
 *   --order hits: traceRays' option order — the rays traced in the order of their first hit points (flx_rays_trace_ordered); the rows are the same
 *   rays.f32: 8 float32 per ray (origin, noise x, direction, noise y); rows.bin: radiance float32[4 n], s float32[n], entry int32[n], transform int32[n],
 *   shades uint32[n].  Without --samples / --bounces / --seed the renderer's defaults apply (config, scene; seed 0); the params used are printed.
 *   --running N: render() runs meanwhile; traceRays is called after every one of its first N frames (the last call's answer is written) and the frames' sums
 *   are printed beside those of the same frames rendered alone.
 *   --filter WxH: the rays are an image of W x H in image order (row 0 on top): renderer.traceImage() traces and DENOISES it (flx_rays_image); rows.bin is then the
 *   image alone, float32[4 n].  --hdr: its tone map (by default config.hdr).
 *   --temporal N (with --filter WxH): the image is accumulated over time (flx_rays_image_temporal) at depth N: traceImage(..., { temporal: true }) is called
 *   --frames F times (by default 1) on history --history H (0) and rows.bin holds the F images one after the other; --chain 0: without the denoise chain;
 *   --reset K: renderer.resetRayHistory(H) before call K.  The seeds are the renderer's own (its counter % N) unless --seed is given.
 *   --camera JSON (with --filter WxH, instead of --rays): a camera description ({} is the engine's own pinhole camera; { "projection": "panorama", ... }:
 *   renderer.cameraOf): traceImage is given the description and the rays are made on the device (flx_camera_image[_temporal]).  --via-rays 1: the rays come back
 *   through renderer.cameraRays() and go in again as a Float32Array, the path the description saves.  --rays-out FILE: cameraRays' rows, float32[8 n].  The camera
 *   the library was given is printed as "camera".
 */
const fs = require('fs');
const path = require('path');
const ROOT = path.resolve(__dirname, '..');
const { FlexLight, Transform } = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'flexlight.js'));
const scenes = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'scenes', 'index.js'));
const sceneFile = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'sceneFile.js'));

const args = process.argv.slice(2);
const name = args[0];
const opt = (flag, d) => { const i = args.indexOf(flag); return i >= 0 ? args[i + 1] : d; };
const sum = a => { let s = 0; for (let i = 0; i < a.length; i++) if (a[i] === a[i]) s += a[i]; return s; };

(async () => {
  const replay = /\.flxs(\.gz)?$/.test(name) ? sceneFile.sceneFromFlxs(path.resolve(name)) : null;
  const frame = replay ? replay.meta.frame : scenes[name].frame;
  Transform.reset();
  const log = console.log; console.log = () => {};
  const canvas = { width: Number(opt('--width', frame.width)), height: Number(opt('--height', frame.height)) };
  const engine = new FlexLight(canvas, { assetRoot: opt('--assets', '/nonexistent') });
  if (replay) {
    engine.scene = replay;
    Object.assign(engine.camera, replay.meta.camera);
    for (let t = 1; t < replay.meta.transforms; t++) new Transform();      // (identity stand-ins, as tools/js_loop.js makes them)
  } else await scenes[name](engine);
  console.log = log;
  engine.config.samplesPerRay = Number(opt('--config-spp', frame.samplesPerRay));
  engine.config.maxReflections = Number(opt('--config-bounces', frame.maxReflections));
  engine.config.filter = false;
  engine.renderer = 'pathtracer';
  const renderer = engine.renderer;
  if (replay) renderer.scene = replay;
  await renderer.updateScene();
  const filterSize = /^(\d+)x(\d+)$/.exec(opt('--filter', ''));
  const description = opt('--camera') !== undefined ? JSON.parse(opt('--camera')) : null;
  if (description && !filterSize) throw new Error('--camera takes --filter WxH');
  const camera = description ? renderer.cameraOf(description, Number(filterSize[1]), Number(filterSize[2])) : null;
  const viaRays = description && Number(opt('--via-rays', 0)) !== 0;
  const madeRays = description && (viaRays || opt('--rays-out') !== undefined) ? renderer.cameraRays(description, Number(filterSize[1]), Number(filterSize[2])) : null;
  if (madeRays && opt('--rays-out') !== undefined) fs.writeFileSync(opt('--rays-out'), Buffer.from(madeRays.buffer, madeRays.byteOffset, madeRays.byteLength));
  const bytes = description ? null : fs.readFileSync(opt('--rays'));
  const rays = description ? (viaRays ? madeRays : description) : new Float32Array(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength));
  const count = description ? Number(filterSize[1]) * Number(filterSize[2]) : rays.length / 8;
  const options = {};
  if (opt('--samples') !== undefined) options.samples = Number(opt('--samples'));
  if (opt('--bounces') !== undefined) options.maxReflections = Number(opt('--bounces'));
  if (opt('--seed') !== undefined) options.randomSeed = Number(opt('--seed'));
  if (opt('--order') !== undefined) options.order = opt('--order');
  const filter = opt('--filter');
  if (filter !== undefined) {
    const size = /^(\d+)x(\d+)$/.exec(filter);
    if (!size) throw new Error('--filter takes WxH');
    if (opt('--hdr') !== undefined) options.hdr = Number(opt('--hdr')) !== 0;
    if (opt('--temporal') !== undefined) {
      options.temporal = true;
      options.temporalSamples = Number(opt('--temporal'));
      options.history = Number(opt('--history', 0));
      options.filter = Number(opt('--chain', 1)) !== 0;
      const frames = Number(opt('--frames', 1)), reset = Number(opt('--reset', -1));
      const images = [];
      for (let f = 0; f < frames; f++) {
        if (f === reset) renderer.resetRayHistory(options.history);
        const image = renderer.traceImage(rays, Number(size[1]), Number(size[2]), options);
        images.push(Buffer.from(image.radiance.buffer, image.radiance.byteOffset, image.radiance.byteLength));
      }
      fs.writeFileSync(opt('--out', 'rows.bin'), Buffer.concat(images));
      console.log(JSON.stringify({ rays: count, camera, width: Number(size[1]), height: Number(size[2]), frames, temporal: options.temporalSamples, history: options.history, chain: options.filter, params: renderer.traceParams(options), hdr: options.hdr === undefined ? !!engine.config.hdr : options.hdr, renderer: renderer.type }));
      renderer.halt();
      return;
    }
    const image = renderer.traceImage(rays, Number(size[1]), Number(size[2]), options);
    fs.writeFileSync(opt('--out', 'rows.bin'), Buffer.from(image.radiance.buffer, image.radiance.byteOffset, image.radiance.byteLength));
    console.log(JSON.stringify({ rays: count, camera, width: image.width, height: image.height, params: renderer.traceParams(options), hdr: options.hdr === undefined ? !!engine.config.hdr : options.hdr, renderer: renderer.type }));
    renderer.halt();
    return;
  }
  const info = { rays: rays.length / 8, order: options.order === undefined ? null : options.order, params: renderer.traceParams(options), config: { samplesPerRay: engine.config.samplesPerRay, maxReflections: engine.config.maxReflections, minImportancy: engine.config.minImportancy }, ambient: Array.from(engine.scene.ambientLight), renderer: renderer.type };
  let rows;
  const running = Number(opt('--running', 0));
  if (running > 0) {
    const alone = renderer.renderFrame();
    info.aloneSum = sum(alone.radiance);
    info.frameSums = [];
    info.errors = 0;
    const error = console.error; console.error = (...a) => { info.errors++; error(...a); };
    await new Promise(resolve => {
      canvas.onFrame = f => {
        info.frameSums.push(sum(f.radiance));
        try { rows = renderer.traceRays(rays, options); } catch (e) { info.errors++; error(e); }
        if (info.frameSums.length >= running) { canvas.onFrame = null; renderer.halt(); setTimeout(resolve, 100); }
      };
      renderer.render();
    });
    console.error = error;
  } else rows = renderer.traceRays(rays, options);
  fs.writeFileSync(opt('--out', 'rows.bin'), Buffer.concat([rows.radiance, rows.s, rows.entry, rows.transform, rows.shades].map(a => Buffer.from(a.buffer, a.byteOffset, a.byteLength))));
  info.hit = Array.from(rows.entry).filter(e => e !== -1).length;
  console.log(JSON.stringify(info));
  renderer.halt();
})().catch(e => { console.error(e); process.exit(1); });
