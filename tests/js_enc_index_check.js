'use strict';
/* js_enc_index_check.js <job.json> -- the indexed compress of the JS front: for the job {cases: [{path, level, spans}]} per case and
 * per form (bytes in and out; stream objects on both sides; bytes without a line table) the digests of the output and of the two
 * tables of Bzip2.compressFileIndexed beside those of Bzip2.compressFile, Bzip2.buildIndex and Bzip2.buildLineIndex on the same
 * bytes, and the bytes of Bzip2.readLines through the returned tables per span (hex), as one JSON line.  Driven by
 * tests/test_gpu_enc_index_js.py. */
var fs = require('fs');
var path = require('path');
var crypto = require('crypto');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function sha(b) { return b === null ? null : crypto.createHash('sha256').update(Buffer.from(b)).digest('hex'); }

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var rep = { cases: [] };
job.cases.forEach(function (c) {
  var data = fs.readFileSync(c.path);
  var plain = Bzip2.compressFile(data, null, c.level);
  var index = Bzip2.buildIndex(plain, false);
  var lineIndex = Bzip2.buildLineIndex(plain, index);
  var r = { plain: sha(plain), index: sha(index), lineIndex: sha(lineIndex), forms: {} };
  function form(name, made, output) {
    r.forms[name] = { output: sha(output), index: sha(made.index), lineIndex: sha(made.lineIndex),
                      spans: made.lineIndex === null ? null : c.spans.map(function (s) {
                        return Buffer.from(Bzip2.readLines(output, made.index, made.lineIndex, s[0], s[1])).toString('hex');
                      }) };
  }
  var a = Bzip2.compressFileIndexed(data, null, c.level);
  form('bytes', a, a.output);
  var pos = 0, chunks = [];
  var inS = { readByte: function () { return pos < data.length ? data[pos++] : -1; },
              read: function (buf, off, len) { var n = Math.min(len, data.length - pos, 300001); data.copy(Buffer.from(buf.buffer, buf.byteOffset + off, n), 0, pos, pos + n); pos += n; return n; } };
  var outS = { writeByte: function (b) { chunks.push(Buffer.from([b])); }, write: function (buf, off, len) { chunks.push(Buffer.from(buf.subarray(off, off + len))); return len; } };
  var b = Bzip2.compressFileIndexed(inS, outS, c.level, {});
  r.returnedSink = b.output === outS;
  form('streams', b, Buffer.concat(chunks));
  var n = Bzip2.compressFileIndexed(data, null, c.level, { lines: false });
  form('noLines', n, n.output);
  rep.cases.push(r);
});
console.log(JSON.stringify(rep));
