'use strict';
/*
 * What sceneFile.buildAtlas costs on the host: the scalar loop the renderers ran over a whole texture list whenever a member changed.
 *   node tools/build_atlas_time.js <n images> <source w> <source h> <cell w> <cell h> [repeats]
 * Random RGBA8 images; two warm-up builds, then `repeats` timed ones.  Prints one JSON line: { ms: [..], width, height }.
 */
const path = require('path');
const sceneFile = require(path.join(__dirname, '..', 'web-ray-tracer_amd', 'js', 'sceneFile.js'));
const [n, sw, sh, w, h, repeats] = process.argv.slice(2).map(Number);
let seed = 12345;
const images = Array.from({ length: n }, () => {
  const data = new Uint8Array(sw * sh * 4);
  for (let i = 0; i < data.length; i++) { seed = (seed * 1103515245 + 12345) & 0x7fffffff; data[i] = seed >> 16; }
  return { width: sw, height: sh, data };
});
const ms = [];
let atlas;
for (let r = 0; r < 2 + (repeats || 7); r++) {
  const t0 = process.hrtime.bigint();
  atlas = sceneFile.buildAtlas(images, [w, h]);
  if (r >= 2) ms.push(Number(process.hrtime.bigint() - t0) / 1e6);
}
console.log(JSON.stringify({ ms, width: atlas.width, height: atlas.height }));
