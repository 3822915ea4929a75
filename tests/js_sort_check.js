'use strict';
/* js_sort_check.js <job.json> -- the line sort of the JS front: for the job {path, multistream, calls: [options], damaged} what
 * Bzip2.sortLines gives per call (the text as hex), then a stream with a damaged block and the refusals.  One JSON line.  Driven by
 * tests/test_gpu_sort_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }
function sort(input, index, table, o) {
  var r = Bzip2.sortLines(input, index, table, o);
  r.lines = Array.from(r.lines);
  r.counts = Array.from(r.counts);
  r.text = r.text === undefined ? null : r.text.toString('hex');
  return r;
}

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var input = fs.readFileSync(job.path);
var index = Bzip2.buildIndex(input, job.multistream);
var table = Bzip2.buildLineIndex(input, index);
var target = fs.readFileSync(job.damaged);
var rep = {
  calls: job.calls.map(function (o) { return attempt(function () { return sort(input, index, table, o); }); }),
  damaged: attempt(function () { return sort(target, index, table, { limit: 5 }); }),
  refusals: {
    fraction: attempt(function () { return sort(input, index, table, { first: 1.5 }); }),
    negative: attempt(function () { return sort(input, index, table, { limit: -2 }); }),
    both: attempt(function () { return sort(input, index, table, { fields: '1', bytes: '2' }); }),
    list: attempt(function () { return sort(input, index, table, { fields: '0' }); }),
    foreign: attempt(function () { return sort(input, index, table.subarray(0, table.length - 4), {}); })
  }
};
console.log(JSON.stringify(rep));
