'use strict';
/* js_cut_check.js <job.json> -- the column cut of the JS front: for the job {cases: [{path, multistream, damaged, calls: [opts]}]}
 * per case what Bzip2.cutLines gives per call (hex), then the refusals.  One JSON line.  Driven by tests/test_gpu_cut_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }
function cut(input, index, table, o) {
  var r = Bzip2.cutLines(input, index, table, o);
  return { isBuffer: Buffer.isBuffer(r), hex: r.toString('hex') };
}

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var rep = { cases: [] };
job.cases.forEach(function (c) {
  var input = fs.readFileSync(c.path);
  var index = Bzip2.buildIndex(input, c.multistream);
  var table = Bzip2.buildLineIndex(input, index);
  var target = c.damaged ? fs.readFileSync(c.damaged) : input;
  rep.cases.push(c.calls.map(function (o) { return attempt(function () { return cut(target, index, table, o); }); }));
  if (!rep.refusals) {
    rep.refusals = {
      neither: attempt(function () { return cut(input, index, table, {}); }),
      both: attempt(function () { return cut(input, index, table, { fields: '1', bytes: '1' }); }),
      wideDelimiter: attempt(function () { return cut(input, index, table, { fields: '1', delimiter: 'ab' }); }),
      zero: attempt(function () { return cut(input, index, table, { fields: '0' }); }),
      notAList: attempt(function () { return cut(input, index, table, { fields: '1,,2' }); }),
      backwards: attempt(function () { return cut(input, index, table, { fields: [[3, 2]] }); }),
      newline: attempt(function () { return cut(input, index, table, { fields: '1', delimiter: '\n' }); }),
      fraction: attempt(function () { return cut(input, index, table, { fields: '1', first: 1.5 }); }),
      foreign: attempt(function () { return cut(input, index, table.subarray(0, table.length - 4), { fields: '1' }); })
    };
  }
});
console.log(JSON.stringify(rep));
