'use strict';
/* js_recover_check.js <jobs.json> -- Bzip2.recoverFile of the JS front on damaged inputs: for every job {name, path} both result
 * forms (sha256, length) and the callback's rows, as one JSON line.  Driven by tests/test_gpu_recover_js.py. */
var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

var jobs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8')), results = [];
jobs.forEach(function (job) {
  var input = fs.readFileSync(job.path), r = { name: job.name, forms: [] };
  [false, true].forEach(function (asStream) {
    var rows = [];
    var out = Bzip2.recoverFile(input, null, function (pos, size, status) { rows.push([pos, size, status]); }, asStream);
    r.forms.push({ isU8: out instanceof Uint8Array, len: out.length, sha256: crypto.createHash('sha256').update(out).digest('hex'), rows: rows });
  });
  // delivered like decompressFile: into a sink with writeByte, and refused when the size is wrong
  var sink = { bytes: [], writeByte: function (b) { this.bytes.push(b); } };
  r.sinkReturned = Bzip2.recoverFile(input, sink) === sink;
  r.sinkLen = sink.bytes.length;
  try { Bzip2.recoverFile(input, 1); r.shortOut = 'no error'; } catch (e) { r.shortOut = e.constructor.name + ':' + e.message; }
  results.push(r);
});
console.log(JSON.stringify({ results: results, shadowed: Bzip2.REC_SHADOWED }));
