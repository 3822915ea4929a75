'use strict';
/* js_range_check.js <job.json> -- the indexed range reads of the JS front: for the job {path, damaged, multistream, ranges, ...} the
 * serialised index of Bzip2.buildIndex (hex), every range of Bzip2.readRanges on the stream and on its damaged copy (hex of the
 * bytes, or the error's class and message), Bzip2.readRange for one good and one failing range, for a stream
 * whose stored block CRC is wrong (crcStream, crcIndex, crcRange) and for a fractional offset and length, as one JSON line.  Driven by
 * tests/test_gpu_range_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function show(x) {
  if (x instanceof Error) { return { error: x.constructor.name + ':' + x.message, code: x.errorCode }; }
  return { isU8: x instanceof Uint8Array, hex: Buffer.from(x).toString('hex') };
}
function attempt(f) { try { return show(f()); } catch (e) { return show(e); } }

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var input = fs.readFileSync(job.path), damaged = fs.readFileSync(job.damaged);
var index = Bzip2.buildIndex(input, job.multistream);
var rep = { indexIsU8: index instanceof Uint8Array, index: Buffer.from(index).toString('hex') };
rep.good = Bzip2.readRanges(input, index, job.ranges).map(show);
rep.bad = Bzip2.readRanges(damaged, index, job.ranges).map(show);
rep.one = attempt(function () { return Bzip2.readRange(input, index, job.ranges[0][0], job.ranges[0][1]); });
rep.oneBad = attempt(function () { return Bzip2.readRange(damaged, index, job.failing[0], job.failing[1]); });
rep.notAnIndex = attempt(function () { return Bzip2.readRange(input, new Uint8Array(40), 0, 1); });
rep.buildBad = attempt(function () { return Bzip2.buildIndex(new Uint8Array([66, 90, 104, 48, 1, 2, 3, 4])); });
rep.crc = attempt(function () { return Bzip2.readRange(fs.readFileSync(job.crcStream), new Uint8Array(Buffer.from(job.crcIndex, 'hex')), job.crcRange[0], job.crcRange[1]); });
rep.fraction = attempt(function () { return Bzip2.readRange(input, index, 10.7, 5); });
rep.fractionLen = attempt(function () { return Bzip2.readRange(input, index, 10, 0.5); });
console.log(JSON.stringify(rep));
