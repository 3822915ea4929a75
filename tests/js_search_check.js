'use strict';
/* js_search_check.js <job.json> -- the pattern search of the JS front: for the job {cases: [{path, multistream, patterns (hex),
 * asStrings, opts, damaged}]} the result of Bzip2.search per case (or the error's class and message), and the refusals of bad
 * arguments, as one JSON line.  Driven by tests/test_gpu_search_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var rep = { cases: [] };
job.cases.forEach(function (c) {
  var input = fs.readFileSync(c.path);
  var index = Bzip2.buildIndex(input, c.multistream);
  var target = c.damaged ? fs.readFileSync(c.damaged) : input;
  var patterns = c.patterns.map(function (h, i) {
    var b = Buffer.from(h, 'hex');
    if (c.asStrings) { return b.toString('latin1'); }             // (ASCII patterns only)
    return i % 2 ? new Uint8Array(b) : b;
  });
  rep.cases.push(attempt(function () { return Bzip2.search(target, index, patterns, c.opts); }));
  if (!rep.refusals) {
    rep.refusals = {
      none: attempt(function () { return Bzip2.search(input, index, [], {}); }),
      empty: attempt(function () { return Bzip2.search(input, index, ['a', ''], {}); }),
      long: attempt(function () { return Bzip2.search(input, index, [Buffer.alloc(257, 97)], {}); }),
      fraction: attempt(function () { return Bzip2.search(input, index, ['a'], { offset: 1.5 }); }),
      notAnIndex: attempt(function () { return Bzip2.search(input, new Uint8Array(40), ['a']); })
    };
  }
});
console.log(JSON.stringify(rep));
