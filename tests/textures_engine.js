'use strict';
/*
 * tests/test_textures_js_gpu.py: the theater scene through the JavaScript renderers, its atlases built by the native uploadTextures / updateTexture.
 *   node textures_engine.js <asset root> <out.f32> pathtracer|rasterizer
 * Writes the first frame (96 x 54, 2 samples, 6 bounces, no filter) and prints one JSON line: the calls a spy on the addon saw for the first frame and for the frame after
 * one member of scene.textures was replaced by an image of another size; whether that frame equals the frame of a fresh engine built with the new list, and of an
 * engine handed atlases composited by sceneFile.buildAtlas (prebuiltAtlases: flx_atlas_upload, the way in before).
 */
const fs = require('fs');
const os = require('os');
const path = require('path');
const childProcess = require('child_process');
const ROOT = path.resolve(__dirname, '..');
const JS = path.join(ROOT, 'web-ray-tracer_amd', 'js');
const { FlexLight, Transform } = require(path.join(JS, 'flexlight.js'));
const scenes = require(path.join(JS, 'scenes', 'index.js'));
const sceneFile = require(path.join(JS, 'sceneFile.js'));
const { native } = require(path.join(JS, 'pathtracerHIP.js'));

const [assets, out, type] = process.argv.slice(2);

function loadImage (rel) {
  const tmp = path.join(os.tmpdir(), 'flx-img-' + process.pid + '.rgba');
  const py = 'import sys; from PIL import Image; im = Image.open(sys.argv[1]).convert("RGBA"); open(sys.argv[2], "wb").write(im.tobytes()); print(im.width, im.height)';
  const dims = childProcess.execFileSync('python3', ['-c', py, path.join(assets, rel), tmp]).toString().trim().split(' ').map(Number);
  const data = new Uint8Array(fs.readFileSync(tmp));
  fs.unlinkSync(tmp);
  return { width: dims[0], height: dims[1], data };
}

// the spy: every atlas call the renderers make on the addon, by name
const addon = native();
let calls = {};
for (const name of ['uploadAtlas', 'uploadTextures', 'updateTexture']) {
  const real = addon[name];
  addon[name] = (...a) => { calls[name] = (calls[name] || 0) + 1; return real(...a); };
}
const taken = () => { const c = calls; calls = {}; return c; };

const holz = loadImage('textures/holz.jpg');
async function engineWith (change) {
  Transform.reset();
  const log = console.log; console.log = () => {};
  const engine = new FlexLight({ width: 96, height: 54 }, { assetRoot: assets });
  engine.loadImage = async () => holz;
  await scenes.theater(engine);
  console.log = log;
  Object.assign(engine.config, { samplesPerRay: 2, maxReflections: 6, filter: false });
  engine.renderer = type;
  if (change) change(engine.scene);
  await engine.renderer.updateScene();
  return engine;
}
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

// another image of another size: 37 x 53, a pattern of its own
const other = { width: 37, height: 53, data: new Uint8Array(37 * 53 * 4) };
for (let i = 0; i < other.data.length; i++) other.data[i] = (i % 4 === 3) ? 255 : (i * 7 + (i >> 5) * 13) & 255;

(async () => {
  const engine = await engineWith(null);
  const first = engine.renderer.renderFrame().radiance.slice();
  const built = taken();
  const again = engine.renderer.renderFrame().radiance.slice();
  const idle = taken();                                              // nothing changed: no atlas call
  fs.writeFileSync(out, Buffer.from(first.buffer, first.byteOffset, first.byteLength));
  engine.scene.textures[0] = other;
  const changed = engine.renderer.renderFrame().radiance.slice();
  const updated = taken();
  const fresh = await engineWith(scene => { scene.textures[0] = other; });
  const freshFrame = fresh.renderer.renderFrame().radiance.slice();
  taken();
  // the way in before: atlases composited by sceneFile.buildAtlas on the host, handed over finished
  const lists = s => [s.textures, s.pbrTextures, s.translucencyTextures].map(l => sceneFile.buildAtlas(l, s.standardTextureSizes));
  const before = await engineWith(scene => { scene.prebuiltAtlases = lists(scene); });
  const beforeFrame = before.renderer.renderFrame().radiance.slice();
  const beforeChanged = await engineWith(scene => { scene.textures[0] = other; scene.prebuiltAtlases = lists(scene); });
  const beforeChangedFrame = beforeChanged.renderer.renderFrame().radiance.slice();
  const prebuilt = taken();
  console.log(JSON.stringify({
    built, idle, updated, prebuilt, stable: same(first, again), frameChanges: !same(first, changed), equalsFresh: same(changed, freshFrame),
    equalsBefore: same(first, beforeFrame), changedEqualsBefore: same(changed, beforeChangedFrame)
  }));
  for (const e of [engine, fresh, before, beforeChanged]) e.renderer.halt();
})().catch(e => { console.error(e); process.exit(1); });
