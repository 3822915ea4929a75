'use strict';
/* js_lines_check.js <job.json> -- the line table of the JS front: for the job {cases: [{path, multistream, lines, offsets, spans,
 * damaged}]} per case the serialised table of Bzip2.buildLineIndex (hex), the results of Bzip2.lineStarts and Bzip2.lineNumbers
 * and the bytes of Bzip2.readLines per span (hex, or the error's class and message), as one JSON line.  Driven by
 * tests/test_gpu_lines_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var rep = { cases: [] };
job.cases.forEach(function (c) {
  var input = fs.readFileSync(c.path);
  var index = Bzip2.buildIndex(input, c.multistream);
  var table = Bzip2.buildLineIndex(input, index);
  var target = c.damaged ? fs.readFileSync(c.damaged) : input;
  rep.cases.push({
    table: Buffer.from(table).toString('hex'),
    starts: attempt(function () { return Bzip2.lineStarts(target, index, table, c.lines); }),
    numbers: attempt(function () { return Bzip2.lineNumbers(target, index, table, c.offsets); }),
    spans: c.spans.map(function (s) { return attempt(function () { return Buffer.from(Bzip2.readLines(target, index, table, s[0], s[1])).toString('hex'); }); })
  });
  if (!rep.refusals) {
    rep.refusals = {
      fraction: attempt(function () { return Bzip2.lineStarts(input, index, table, [1.5]); }),
      negative: attempt(function () { return Bzip2.lineNumbers(input, index, table, [-1]); }),
      notATable: attempt(function () { return Bzip2.lineStarts(input, index, new Uint8Array(48), [1]); }),
      foreign: attempt(function () { return Bzip2.lineStarts(input, index, table.subarray(0, table.length - 4), [1]); }),
      damagedBuild: c.damaged ? attempt(function () { return Bzip2.buildLineIndex(target, index); }) : null
    };
  }
});
console.log(JSON.stringify(rep));
