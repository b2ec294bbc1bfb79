'use strict';
// The yardstick of tests/test_textures_cpu.py: sceneFile.buildAtlas over images given as raw RGBA8 files.
// usage: node textures_build_atlas.js spec.json — spec = { cell: [w, h], images: [{ width, height, file }], out }; prints { width, height }
const fs = require('fs');
const path = require('path');
const sceneFile = require(path.join(__dirname, '..', 'web-ray-tracer_amd', 'js', 'sceneFile.js'));

const spec = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const images = spec.images.map(i => ({ width: i.width, height: i.height, data: new Uint8Array(fs.readFileSync(i.file)) }));
const atlas = sceneFile.buildAtlas(images, spec.cell);
fs.writeFileSync(spec.out, Buffer.from(atlas.data.buffer, atlas.data.byteOffset, atlas.data.byteLength));
console.log(JSON.stringify({ width: atlas.width, height: atlas.height }));
