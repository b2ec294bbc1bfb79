'use strict';
/*
 * A ray IMAGE traced WITH A PROBE VOLUME through a BASELINE scene by the whole JavaScript path — FlexLight facade, scene graph, host flattening, N-API addon,
 * libflexlight_hip.so (flx_volume_bake_device, flx_rays_image_gather and its kin) — and what renderer.traceImage(raysOrCamera, width, height, { volume, gain })
 * returns in its four forms: rays or a camera, with and without temporal.
 *   node tools/trace_image_gather.js <scene> --size WxH --origin x,y,z --spacing x,y,z --count nx,ny,nz --dir DIR
 *                                    [--map size,sharpness --relocate backShare,minFront,reach,limit,iterations,faceSize --face W --gain G
 *                                     --samples S --bounces B --seed X --bias b --depth N --nofilter]
 *   DIR/rays.f32                      the engine's own pinhole camera's rays, renderer.cameraRays({}, W, H): 8 float32 per ray
 *   DIR/rays.bin, DIR/camera.bin      traceImage(rays, W, H, { volume }) and traceImage({}, W, H, { volume }): float32[4 W H]
 *   DIR/rays_temporal.bin, DIR/camera_temporal.bin   the second of two frames with { temporal: true } on histories 0 and 1, seeds X and X + 1
 *   DIR/plain.bin                     traceImage(rays, W, H) without a volume
 *   DIR/rows.bin [maps.bin] [offsets.bin]   the volume's SH rows, its maps and its offsets as they stand on the device
 *   The last line printed is JSON: the grid, the trace params, the gain the calls used, the transform arrays, and which TypeErrors were thrown.
 */
const fs = require('fs');
const path = require('path');
const ROOT = path.resolve(__dirname, '..');
const { FlexLight, Transform } = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'flexlight.js'));
const scenes = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'scenes', 'index.js'));

const args = process.argv.slice(2);
const name = args[0];
const opt = (flag, d) => { const i = args.indexOf(flag); return i >= 0 ? args[i + 1] : d; };
const three = (flag) => opt(flag).split(',').map(Number);
const dir = opt('--dir', '.');
const write = (file, a) => fs.writeFileSync(path.join(dir, file), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const thrown = f => { try { f(); } catch (e) { return e instanceof TypeError ? 'TypeError' : e instanceof Error ? 'Error' : 'other'; } return null; };

(async () => {
  Transform.reset();
  const [width, height] = opt('--size', '40x27').split('x').map(Number);
  const log = console.log; console.log = () => {};
  const engine = new FlexLight({ width, height }, { assetRoot: opt('--assets', '/nonexistent') });
  await scenes[name](engine);
  console.log = log;
  engine.config.samplesPerRay = Number(opt('--samples', 1));
  engine.config.maxReflections = Number(opt('--bounces', 2));
  engine.renderer = 'pathtracer';
  const renderer = engine.renderer;
  await renderer.updateScene();
  const rays = renderer.cameraRays({}, width, height);
  write('rays.f32', rays);
  const grid = { origin: three('--origin'), spacing: three('--spacing'), count: three('--count') };
  if (opt('--bias') !== undefined) grid.normalBias = Number(opt('--bias'));
  const bake = { faceSize: Number(opt('--face', 4)) };
  const seed = Number(opt('--seed', 0));
  bake.randomSeed = seed;
  if (opt('--map') !== undefined) { const m = opt('--map').split(',').map(Number); bake.map = { size: m[0], sharpness: m[1] }; }
  if (opt('--relocate') !== undefined) {
    const r = opt('--relocate').split(',').map(Number);
    bake.relocate = { backShare: r[0], minFront: r[1], reach: r[2], limit: r[3], iterations: r[4], faceSize: r[5] };
  }
  const volume = renderer.bakeVolume(grid, bake);
  write('rows.bin', volume.rows());
  if (volume.maps) write('maps.bin', volume.maps());
  if (volume.offsets) write('offsets.bin', volume.offsets());
  const options = { volume, hdr: true, randomSeed: seed };
  if (opt('--gain') !== undefined) options.gain = Number(opt('--gain'));
  write('rays.bin', renderer.traceImage(rays, width, height, options).radiance);
  write('camera.bin', renderer.traceImage({}, width, height, options).radiance);
  const depth = Number(opt('--depth', 3)), filter = args.indexOf('--nofilter') < 0;
  renderer.resetRayHistory();
  const over = (history, k) => Object.assign({}, options, { temporal: true, history, temporalSamples: depth, filter, randomSeed: seed + k });
  renderer.traceImage(rays, width, height, over(0, 0));
  write('rays_temporal.bin', renderer.traceImage(rays, width, height, over(0, 1)).radiance);
  renderer.traceImage({}, width, height, over(1, 0));
  write('camera_temporal.bin', renderer.traceImage({}, width, height, over(1, 1)).radiance);
  const without = Object.assign({}, options);
  delete without.volume;
  write('plain.bin', renderer.traceImage(rays, width, height, without).radiance);
  const errors = {
    notAHandle: thrown(() => renderer.traceImage(rays, width, height, { volume: { grid } })),
    nullVolume: thrown(() => renderer.traceImage(rays, width, height, { volume: null })),
    numberVolume: thrown(() => renderer.traceImage({}, width, height, { volume: 7 })),
    foreignHandle: thrown(() => renderer.traceImage(rays, width, height, { volume: { _handle: {} } })),
    gainString: thrown(() => renderer.traceImage(rays, width, height, { volume, gain: '1' })),
    gainStringTemporal: thrown(() => renderer.traceImage({}, width, height, { volume, gain: '1', temporal: true })),
    gainNegative: thrown(() => renderer.traceImage(rays, width, height, { volume, gain: -1 })),
    group: (() => { const saved = renderer._devices; renderer._devices = [0, 0]; const e = thrown(() => renderer.traceImage(rays, width, height, { volume })); renderer._devices = saved; return e; })()
  };
  const tr = Transform.buildWGL2Arrays();
  console.log(JSON.stringify({ width, height, probes: volume.probes, grid: volume.grid, trace: renderer.traceParams(options), gain: options.gain === undefined ? Math.fround(1 / Math.PI) : options.gain,
    depth, filter, seed, rotation: Array.from(tr[0]), shift: Array.from(tr[1]), map: volume.map === undefined ? null : volume.map, hasOffsets: volume.offsets !== undefined,
    errors, renderer: renderer.type }));
  renderer.halt();
})().catch(e => { console.error(e); process.exit(1); });
