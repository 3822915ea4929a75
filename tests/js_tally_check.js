'use strict';
/* js_tally_check.js <job.json> -- the line frequency table of the JS front: for the job {path, multistream, calls: [options]} what
 * Bzip2.tallyLines gives per call (the groups as hex), then the refusals.  One JSON line.  Driven by tests/test_gpu_tally_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }
function tally(input, index, table, o) {
  var r = Bzip2.tallyLines(input, index, table, o);
  r.groups = Buffer.from(r.groups).toString('hex');
  return r;
}

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var input = fs.readFileSync(job.path);
var index = Bzip2.buildIndex(input, job.multistream);
var table = Bzip2.buildLineIndex(input, index);
var target = job.damaged ? fs.readFileSync(job.damaged) : null;
var rep = {
  calls: job.calls.map(function (o) { return attempt(function () { return tally(input, index, table, o); }); }),
  damaged: target ? attempt(function () { return tally(target, index, table, { limit: 5 }); }) : null,
  damagedCut: target ? attempt(function () { return tally(target, index, table, { fields: '2', limit: 5 }); }) : null,
  refusals: {
    fraction: attempt(function () { return tally(input, index, table, { first: 1.5 }); }),
    negative: attempt(function () { return tally(input, index, table, { minCount: -1 }); }),
    both: attempt(function () { return tally(input, index, table, { fields: '1', bytes: '2' }); }),
    order: attempt(function () { return tally(input, index, table, { order: 'content' }); }),
    filter: attempt(function () { return tally(input, index, table, { minCount: 3, maxCount: 2 }); }),
    foreign: attempt(function () { return tally(input, index, table.subarray(0, table.length - 4), {}); })
  }
};
console.log(JSON.stringify(rep));
