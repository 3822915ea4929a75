'use strict';
/* js_linekeys_check.js <job.json> -- the line keys of the JS front: for the job {cases: [{path, multistream, windows, seed, other,
 * damaged}]} per case the records of Bzip2.lineKeys per window (hex) and, with `other` (a second stream), what Bzip2.diffLines
 * gives against it; then the refusals.  One JSON line.  Driven by tests/test_gpu_linekeys_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }
function keys(input, index, table, o) {
  var r = Bzip2.lineKeys(input, index, table, o);
  r.keys = Buffer.from(r.keys).toString('hex');
  return r;
}

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var rep = { cases: [] };
job.cases.forEach(function (c) {
  var input = fs.readFileSync(c.path);
  var index = Bzip2.buildIndex(input, c.multistream);
  var table = Bzip2.buildLineIndex(input, index);
  var target = c.damaged ? fs.readFileSync(c.damaged) : input;
  var out = { windows: c.windows.map(function (w) { return attempt(function () { return keys(target, index, table, { first: w[0], count: w[1] === null ? undefined : w[1], seed: c.seed }); }); }) };
  if (c.other) {
    var other = fs.readFileSync(c.other), oIndex = Bzip2.buildIndex(other, false), oTable = Bzip2.buildLineIndex(other, oIndex);
    out.diff = attempt(function () { return Bzip2.diffLines(target, index, table, other, oIndex, oTable, { seed: c.seed }); });
    out.diffCapped = attempt(function () { return Bzip2.diffLines(target, index, table, other, oIndex, oTable, { seed: c.seed, maxEdits: 2 }); });
    out.same = attempt(function () { return Bzip2.diffLines(other, oIndex, oTable, other, oIndex, oTable); });
  }
  rep.cases.push(out);
  if (!rep.refusals) {
    rep.refusals = {
      fraction: attempt(function () { return keys(input, index, table, { first: 1.5 }); }),
      negative: attempt(function () { return keys(input, index, table, { seed: -1 }); }),
      notATable: attempt(function () { return keys(input, index, new Uint8Array(48), {}); }),
      foreign: attempt(function () { return keys(input, index, table.subarray(0, table.length - 4), {}); })
    };
  }
});
console.log(JSON.stringify(rep));
