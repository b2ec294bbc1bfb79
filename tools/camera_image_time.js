'use strict';
/*
 * What renderer.traceImage() costs the host for a 1080p panorama, by the whole JavaScript path — FlexLight facade, scene graph, N-API addon, libflexlight_hip.so:
 *   rays built in JavaScript + traceImage(Float32Array)   what an application did before the library had cameras: 2 073 600 rays of 8 floats computed per pixel in
 *                                                         JavaScript, 66 MB over N-API and PCIe, 33 MB of image back
 *   traceImage(Float32Array), the rays built before       the same call with the array at hand (an application that keeps its rays from image to image)
 *   traceImage(description)                               the camera path: the rays made on the device (flx_camera_image), 33 MB of image back
 * on the same scene and parameters.  Host milliseconds per call (the calls wait for their answer), the three in turn, round after round, median of --repeats rounds
 * after 2 warm-up rounds [min .. max].  Once, outside the timed region: traceImage(description) equals traceImage(cameraRays(description)) byte for byte.  GPU box.
 *   node tools/camera_image_time.js [scene] [--repeats 10] [--size WxH] [--spp 4] [--bounces 3] [--temporal 1] [--out FILE]      (recorded in profiles/camera_rays.txt)
 */
const fs = require('fs');
const path = require('path');
const ROOT = path.resolve(__dirname, '..');
const { FlexLight, Transform } = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'flexlight.js'));
const scenes = require(path.join(ROOT, 'web-ray-tracer_amd', 'js', 'scenes', 'index.js'));

const args = process.argv.slice(2);
const name = args[0] && !args[0].startsWith('--') ? args[0] : 'cornell';
const opt = (flag, d) => { const i = args.indexOf(flag); return i >= 0 ? args[i + 1] : d; };
const size = /^(\d+)x(\d+)$/.exec(opt('--size', '1920x1080'));
const W = Number(size[1]), H = Number(size[2]), REPEATS = Number(opt('--repeats', 10)), WARMUP = 2;
const temporal = Number(opt('--temporal', 0)) !== 0;

/* an equirectangular camera's rays as an application writes them: per pixel, in JavaScript's doubles, into traceRays' rows */
function panoramaRays (position, basis, extent, width, height) {
  const rays = new Float32Array(8 * width * height);
  for (let row = 0, k = 0; row < height; row++) {
    const sy = (height - 1 - row + 0.5) / height * 2 - 1, lat = sy * 0.5 * extent[1];
    const sinLat = Math.sin(lat), cosLat = Math.cos(lat);
    for (let px = 0; px < width; px++, k += 8) {
      const sx = (px + 0.5) / width * 2 - 1, lon = sx * 0.5 * extent[0];
      const lx = Math.sin(lon) * cosLat, lz = Math.cos(lon) * cosLat;
      const x = basis[0] * lx + basis[3] * sinLat + basis[6] * lz, y = basis[1] * lx + basis[4] * sinLat + basis[7] * lz, z = basis[2] * lx + basis[5] * sinLat + basis[8] * lz;
      const len = Math.sqrt(x * x + y * y + z * z);
      rays[k] = position[0]; rays[k + 1] = position[1]; rays[k + 2] = position[2]; rays[k + 3] = sx;
      rays[k + 4] = x / len; rays[k + 5] = y / len; rays[k + 6] = z / len; rays[k + 7] = sy;
    }
  }
  return rays;
}

(async () => {
  const frame = scenes[name].frame;
  Transform.reset();
  const log = console.log; console.log = () => {};
  const engine = new FlexLight({ width: frame.width, height: frame.height }, { assetRoot: opt('--assets', '/nonexistent') });
  await scenes[name](engine);
  console.log = log;
  engine.config.samplesPerRay = Number(opt('--spp', 4));
  engine.config.maxReflections = Number(opt('--bounces', 3));
  engine.renderer = 'pathtracer';
  const renderer = engine.renderer;
  await renderer.updateScene();
  const description = { projection: 'panorama', basis: [0.8, 0, -0.6, 0, 1, 0, 0.6, 0, 0.8] };
  const camera = renderer.cameraOf(description, W, H);
  const options = temporal ? { temporal: true, temporalSamples: 4 } : {};
  const built = panoramaRays(camera.position, camera.basis, camera.extent, W, H);
  /* once, outside the timed region */
  const made = renderer.cameraRays(description, W, H);
  if (temporal) renderer.resetRayHistory();
  const a = renderer.traceImage(description, W, H, options).radiance;
  if (temporal) renderer.resetRayHistory();
  const b = renderer.traceImage(made, W, H, options).radiance;
  if (Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) !== 0) throw new Error('the camera image is not the ray image of the generated rays');
  let worst = 0;
  for (let k = 0; k < built.length; k++) worst = Math.max(worst, Math.abs(built[k] - made[k]));
  const calls = [
    ['rays built in JavaScript + traceImage(Float32Array)', () => renderer.traceImage(panoramaRays(camera.position, camera.basis, camera.extent, W, H), W, H, options)],
    ['traceImage(Float32Array), the rays built before', () => renderer.traceImage(built, W, H, options)],
    ['traceImage(description)', () => renderer.traceImage(description, W, H, options)]
  ];
  const ms = calls.map(() => []);
  for (let k = 0; k < WARMUP + REPEATS; k++) {
    calls.forEach(([, call], i) => {
      const t0 = process.hrtime.bigint();
      call();
      const t1 = process.hrtime.bigint();
      if (k >= WARMUP) ms[i].push(Number(t1 - t0) / 1e6);
    });
  }
  const median = v => { const s = v.slice().sort((x, y) => x - y); return s.length % 2 ? s[(s.length - 1) / 2] : (s[s.length / 2 - 1] + s[s.length / 2]) / 2; };
  const lines = ['renderer.traceImage, a ' + W + ' x ' + H + ' panorama of ' + name + ', ' + engine.config.samplesPerRay + ' spp, ' + engine.config.maxReflections + ' bounces' + (temporal ? ', { temporal: true }' : '') +
                 '; host ms per call, the calls in turn, median of ' + REPEATS + ' rounds after ' + WARMUP + ' warm-up rounds [min .. max]'];
  calls.forEach(([label], i) => lines.push('  ' + label.padEnd(54) + median(ms[i]).toFixed(3).padStart(10) + ' ms [' + Math.min(...ms[i]).toFixed(3).padStart(10) + ' .. ' + Math.max(...ms[i]).toFixed(3).padStart(10) + ']'));
  lines.push('  verified once outside the timed region: traceImage(description) equals traceImage(cameraRays(description)) byte for byte; the rays built in JavaScript differ from the device\'s by at most ' + worst.toExponential(2) + ' in a word');
  if (opt('--out') !== undefined) fs.writeFileSync(opt('--out'), lines.join('\n') + '\n');
  console.log(lines.join('\n'));
  renderer.halt();
})().catch(e => { console.error(e); process.exit(1); });
