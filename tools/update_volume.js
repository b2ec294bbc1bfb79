'use strict';
/*
 * A probe volume of a BASELINE scene baked and then UPDATED by the whole JavaScript path — FlexLight facade, scene graph, host flattening, N-API addon,
 * libflexlight_hip.so (flx_volume_bake_device or flx_volume_bake_map_device, then flx_volume_update_device) — and write what renderer.updateVolume() leaves in the
 * handle's rows and maps and the states it returns.
 *   node tools/update_volume.js <scene> --origin x,y,z --spacing x,y,z --count nx,ny,nz --rows rows.bin --states states.bin [--maps maps.bin --map size,sharpness
 *                              --face W --sky r,g,b --config-spp S --config-bounces B --seed X]
 *                              --update h,seed,i0:i1:..  |  --update h,seed,first+stride*count   (any number of them, run in the order given)
 *   rows.bin: 36 float32 per probe after the last update; maps.bin: 4 float32 per bin of every probe; states.bin: the uint32 states of all updates, one after the other.
 *   The last line printed is JSON: the grid, the trace params of the bake, the updates as they were understood and the transform arrays the renderer used, so that a
 *   caller can repeat the calls.
 */
const fs = require('fs');
const path = require('path');
const ROOT = path.resolve(__dirname, '..');
const { FlexLight, Transform } = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'flexlight.js'));
const scenes = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'scenes', 'index.js'));

const args = process.argv.slice(2);
const name = args[0];
const opt = (flag, d) => { const i = args.indexOf(flag); return i >= 0 ? args[i + 1] : d; };
const all = (flag) => args.map((a, i) => (a === flag ? args[i + 1] : undefined)).filter(a => a !== undefined);
const three = (flag) => opt(flag).split(',').map(Number);
const write = (file, a) => fs.writeFileSync(file, Buffer.from(a.buffer, a.byteOffset, a.byteLength));

(async () => {
  Transform.reset();
  const log = console.log; console.log = () => {};
  const engine = new FlexLight({ width: 64, height: 48 }, { assetRoot: opt('--assets', '/nonexistent') });
  await scenes[name](engine);
  console.log = log;
  engine.config.samplesPerRay = Number(opt('--config-spp', 1));
  engine.config.maxReflections = Number(opt('--config-bounces', 1));
  engine.config.filter = false;
  engine.renderer = 'pathtracer';
  const renderer = engine.renderer;
  await renderer.updateScene();
  const grid = { origin: three('--origin'), spacing: three('--spacing'), count: three('--count') };
  const options = { faceSize: Number(opt('--face', 8)) };
  if (opt('--seed') !== undefined) options.randomSeed = Number(opt('--seed'));
  if (opt('--sky') !== undefined) options.sky = opt('--sky').split(',').map(Number);
  if (opt('--map') !== undefined) { const m = opt('--map').split(',').map(Number); options.map = { size: m[0], sharpness: m[1] }; }
  const volume = renderer.bakeVolume(grid, options);
  const updates = [];
  const states = [];
  for (const text of all('--update')) {
    const [h, seed, list] = text.split(',');
    let probes;
    if (list.includes('+')) {
      const [first, rest] = list.split('+');
      const [stride, count] = rest.split('*');
      probes = { first: Number(first), stride: Number(stride), count: Number(count) };
    } else probes = Uint32Array.from(list.split(':').map(Number));
    const got = renderer.updateVolume(volume, { hysteresis: Number(h), randomSeed: Number(seed), probes });
    states.push(...got.states);
    updates.push({ hysteresis: Number(h), seed: Number(seed), probes: probes instanceof Uint32Array ? Array.from(probes) : probes, states: Array.from(got.states) });
  }
  write(opt('--rows', 'rows.bin'), volume.rows());
  if (volume.maps) write(opt('--maps', 'maps.bin'), volume.maps());
  write(opt('--states', 'states.bin'), Uint32Array.from(states));
  const tr = Transform.buildWGL2Arrays();
  console.log(JSON.stringify({ probes: volume.probes, grid: volume.grid, faceSize: options.faceSize, trace: renderer.traceParams(options), updates, rotation: Array.from(tr[0]),
    shift: Array.from(tr[1]), renderer: renderer.type, map: volume.map === undefined ? null : volume.map }));
  renderer.halt();
})().catch(e => { console.error(e); process.exit(1); });
