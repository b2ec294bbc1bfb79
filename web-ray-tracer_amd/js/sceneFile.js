'use strict';
/*
 * Assemble the complete render input of one frame (SURVEY.md §8a rows D1–D7) from a FlexLight
 * scene graph and store it as a .flxs file.  Used by tools/make_scenes.js (this repo's host
 * layer) and by tools/ref_goldens.js (arrays emitted by the reference's own scene.js).
 */
const flxs = require('./flxs.js');

// Light array as the reference uploads it (modules/pathtracerWGL2.js:143-165): per light
// [x, y, z, intensity, variation, 0]; a missing intensity/variation property takes the scene default.
function buildLightArray (scene) {
  const lights = scene.primaryLightSources;
  const out = new Float32Array(6 * lights.length);
  lights.forEach((l, i) => {
    const intensity = l.intensity === undefined ? scene.defaultLightIntensity : l.intensity;
    const variation = l.variation === undefined ? scene.defaultLightVariation : l.variation;
    out.set([l[0], l[1], l[2], intensity, variation, 0], i * 6);
  });
  return out;
}

// Atlas as modules/pathtracerWGL2.js:85-104 draws it: every source image nearest-resampled to
// standardTextureSizes and placed at column i % tw, row floor(i / tw); the canvas is
// width*tw by height*list.length (taller than needed; unused cells stay transparent black).
// `images` are {width, height, data: Uint8Array RGBA}.  Nearest resample rule (the browser's is
// unspecified; this is the definition here): destination pixel centre -> floor of source coordinate.
function buildAtlas (images, sizes) {
  if (images.length === 0) return { width: 1, height: 1, data: new Uint8Array(4) };
  const w = sizes[0], h = sizes[1];
  const tw = Math.floor(2048 / w);
  const W = w * tw, H = h * images.length;
  const data = new Uint8Array(W * H * 4);
  images.forEach((img, i) => {
    const ox = w * (i % tw), oy = h * Math.floor(i / tw);
    for (let y = 0; y < h; y++) {
      const sy = Math.min(img.height - 1, Math.floor((y + 0.5) * img.height / h));
      for (let x = 0; x < w; x++) {
        const sx = Math.min(img.width - 1, Math.floor((x + 0.5) * img.width / w));
        const s = (sy * img.width + sx) * 4, d = ((oy + y) * W + ox + x) * 4;
        data[d] = img.data[s]; data[d + 1] = img.data[s + 1]; data[d + 2] = img.data[s + 2]; data[d + 3] = img.data[s + 3];
      }
    }
  });
  return { width: W, height: H, data };
}

// An image of a texture list as the native uploadTextures / updateTexture take it: the width * height * 4 bytes buildAtlas reads of img.data (anything that is no
// byte array converted as buildAtlas' store into its Uint8Array converts it; missing bytes are 0).  The native atlas is then buildAtlas' byte for byte.
function nativeTexture (img) {
  const n = img.width * img.height * 4;
  let data = img.data;
  if (!(data instanceof Uint8Array || data instanceof Uint8ClampedArray)) data = Uint8Array.from(data);
  if (data.length !== n) { const d = new Uint8Array(n); d.set(data.subarray(0, Math.min(n, data.length))); data = d; }
  return { width: img.width, height: img.height, data };
}

// viewMatrix of modules/pathtracerWGL2.js:312-318 (row-major, uploaded with transpose = true).
function buildViewMatrix (camera, width, height) {
  const invFov = 1 / camera.fov;
  const k = height * invFov / width;
  const fx = camera.fx, fy = camera.fy;
  return new Float32Array([
    Math.cos(fx) * k, 0, Math.sin(fx) * k,
    -Math.sin(fx) * Math.sin(fy) * invFov, Math.cos(fy) * invFov, Math.cos(fx) * Math.sin(fy) * invFov,
    -Math.sin(fx) * Math.cos(fy), -Math.sin(fy), Math.cos(fx) * Math.cos(fy)
  ]);
}

function assemble (name, engine, built, transformArrays, frame, extraMeta) {
  const scene = engine.scene, camera = engine.camera;
  const sizes = scene.standardTextureSizes;
  const albedo = buildAtlas(scene.textures, sizes);
  const pbr = buildAtlas(scene.pbrTextures, sizes);
  const tpo = buildAtlas(scene.translucencyTextures, sizes);
  const meta = Object.assign({
    name,
    textureLength: built.textureLength,
    bufferLength: built.bufferLength,
    entriesPadded: built.geometryBuffer.length / 12,
    transforms: transformArrays[1].length / 8,
    lights: scene.primaryLightSources.length,
    camera: { x: camera.x, y: camera.y, z: camera.z, fx: camera.fx, fy: camera.fy, fov: camera.fov },
    ambient: Array.from(scene.ambientLight),
    textureWidth: Math.floor(2048 / sizes[0]),
    atlas: {
      albedo: [albedo.width, albedo.height], pbr: [pbr.width, pbr.height], tpo: [tpo.width, tpo.height]
    },
    frame
  }, extraMeta || {});
  const arrays = {
    geometry: built.geometryBuffer,
    attributes: built.sceneBuffer,
    ids: built.idBuffer,
    rotation: transformArrays[0],
    shift: transformArrays[1],
    lights: buildLightArray(scene),
    viewMatrix: buildViewMatrix(camera, frame.width, frame.height),
    atlasAlbedo: albedo.data,
    atlasPbr: pbr.data,
    atlasTpo: tpo.data
  };
  return { meta, arrays };
}

function save (file, name, engine, built, transformArrays, frame, extraMeta) {
  const s = assemble(name, engine, built, transformArrays, frame, extraMeta);
  flxs.write(file, s.meta, s.arrays);
  return s;
}

/* A scene that replays a .flxs file: what the renderer asks of a Scene (generateArraysFromGraph, light list, ambient light, texture
 * lists, standardTextureSizes) answered from the stored arrays — for boxes without the OBJ / JPEG assets (the GPU box).  The
 * atlases come prebuilt (`prebuiltAtlases`); transforms are NOT replayed: the caller re-creates its Transform objects, so that
 * an animation can move them (tools/js_loop.js). */
function sceneFromFlxs (file) {
  const { meta, arrays } = flxs.read(file);
  const lights = [];
  for (let i = 0; i < arrays.lights.length; i += 6) {
    const l = [arrays.lights[i], arrays.lights[i + 1], arrays.lights[i + 2]];
    l.intensity = arrays.lights[i + 3]; l.variation = arrays.lights[i + 4];
    lights.push(l);
  }
  const atlas = k => ({ width: meta.atlas[k][0], height: meta.atlas[k][1], data: arrays['atlas' + k[0].toUpperCase() + k.slice(1)] });
  return {
    meta,
    primaryLightSources: lights, defaultLightIntensity: 200, defaultLightVariation: 0.4,
    ambientLight: meta.ambient.slice(),
    textures: [], pbrTextures: [], translucencyTextures: [],
    standardTextureSizes: [Math.floor(2048 / meta.textureWidth), Math.floor(2048 / meta.textureWidth)],
    prebuiltAtlases: [atlas('albedo'), atlas('pbr'), atlas('tpo')],
    queue: [],
    generateArraysFromGraph: () => ({ textureLength: meta.textureLength, bufferLength: meta.bufferLength, geometryBuffer: arrays.geometry, sceneBuffer: arrays.attributes, idBuffer: arrays.ids })
  };
}

/* Which rows of the flattened scene changed between two generateArraysFromGraph() results — for flx_scene_update, which takes rows whose
 * vertices or attributes moved and refits the boxes on the device.  null: the row path does not apply — no earlier arrays (or the very same
 * array objects: nothing to compare with), different lengths, different ids, a difference in what fixes the topology (word 10, the kind, of any
 * row; word 9, the transform number, of a box or triangle; word 6, the skip count, of a box), or a vertex in the span that is not finite (the
 * library refuses those).  Otherwise {first, count}: the ONE span from the first to the last differing row; count 0 when nothing differs.
 * Words 0..5 of a box row do not count: they follow from the vertices, and the device computes them.  Compared as bits. */
function changedRows (oldBuilt, newBuilt) {
  if (!oldBuilt || !newBuilt) return null;
  const g0 = oldBuilt.geometryBuffer, g1 = newBuilt.geometryBuffer, a0 = oldBuilt.sceneBuffer, a1 = newBuilt.sceneBuffer;
  const i0 = oldBuilt.idBuffer, i1 = newBuilt.idBuffer;
  if (g0 === g1 || a0 === a1) return null;
  if (g0.length !== g1.length || a0.length !== a1.length || i0.length !== i1.length || g0.length % 12 !== 0 || a0.length / 28 !== g0.length / 12) return null;
  for (let i = 0; i < i0.length; i++) if (i0[i] !== i1[i]) return null;
  const words = f => new Int32Array(f.buffer, f.byteOffset, f.length);
  const G0 = words(g0), G1 = words(g1), A0 = words(a0), A1 = words(a1);
  const n = g0.length / 12;
  const rowDiffers = r => {
    const g = r * 12, a = r * 28;
    for (let k = g1[g + 10] === 1 ? 6 : 0; k < 12; k++) if (G0[g + k] !== G1[g + k]) return true;
    for (let k = 0; k < 28; k++) if (A0[a + k] !== A1[a + k]) return true;
    return false;
  };
  for (let r = 0; r < n; r++) {
    const g = r * 12;
    if (G0[g + 10] !== G1[g + 10]) return null;
    const kind = g1[g + 10];
    if (kind !== 0 && G0[g + 9] !== G1[g + 9]) return null;
    if (kind === 1 && G0[g + 6] !== G1[g + 6]) return null;
  }
  let first = 0, last = n - 1;
  while (first < n && !rowDiffers(first)) first++;
  if (first === n) return { first: 0, count: 0 };
  while (!rowDiffers(last)) last--;
  for (let r = first; r <= last; r++) {
    if (g1[r * 12 + 10] !== 2) continue;
    for (let k = 0; k < 9; k++) if (!Number.isFinite(g1[r * 12 + k])) return null;
  }
  return { first, count: last - first + 1 };
}

module.exports = { buildLightArray, buildAtlas, nativeTexture, buildViewMatrix, assemble, save, sceneFromFlxs, changedRows };
