'use strict';
/* js_compare_check.js <job.json> -- the compare of the JS front: for the job {cases: [{path, multistream, other (a file of plain
 * bytes) or otherStream (a .bz2 file), opts, damaged}]} the result of Bzip2.compare / Bzip2.compareStreams per case (or the
 * error's class and message), and the refusals of bad arguments, as one JSON line.  Driven by tests/test_gpu_compare_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var rep = { cases: [] };
job.cases.forEach(function (c, i) {
  var input = fs.readFileSync(c.path);
  var index = Bzip2.buildIndex(input, c.multistream);
  var target = c.damaged ? fs.readFileSync(c.damaged) : input;
  if (c.otherStream) {
    var b = fs.readFileSync(c.otherStream);
    var indexB = Bzip2.buildIndex(b, false);
    rep.cases.push(attempt(function () { return Bzip2.compareStreams(target, index, b, indexB, c.opts); }));
  } else {
    var other = fs.readFileSync(c.other);
    if (c.slice) { other = other.subarray(c.slice[0], c.slice[1]); }
    rep.cases.push(attempt(function () { return Bzip2.compare(target, index, i % 2 ? new Uint8Array(other) : other, c.opts); }));
  }
  if (!rep.refusals) {
    rep.refusals = {
      fraction: attempt(function () { return Bzip2.compare(input, index, new Uint8Array(4), { offset: 1.5 }); }),
      negative: attempt(function () { return Bzip2.compare(input, index, new Uint8Array(4), { otherOffset: -1 }); }),
      notAnIndex: attempt(function () { return Bzip2.compare(input, new Uint8Array(40), new Uint8Array(4)); }),
      otherIndex: attempt(function () { return Bzip2.compareStreams(input, index, input, new Uint8Array(40)); }),
      wrongStream: attempt(function () { return Bzip2.compare(input.subarray(1), index, new Uint8Array(4)); })
    };
  }
});
console.log(JSON.stringify(rep));
