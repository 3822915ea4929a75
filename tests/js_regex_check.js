'use strict';
/* js_regex_check.js <job.json> -- the regex search of the JS front: for the job {cases: [{path, multistream, patterns (hex),
 * asStrings, opts, damaged}], check: [patterns (hex)]} the result of Bzip2.searchRegex per case (or the error's class and message),
 * Bzip2.regexCheck of `check` with and without nocase, and the refusals of bad patterns and arguments, as one JSON line.  Driven by
 * tests/test_gpu_regex_js.py. */
var fs = require('fs');
var path = require('path');
var Bzip2 = require(path.join(__dirname, '..', 'compressjs-flattened_amd', 'js', 'Bzip2.js'));

function attempt(f) { try { return f(); } catch (e) { return { error: e.constructor.name + ':' + e.message, code: e.errorCode }; } }
function unhex(list, asStrings) {
  return list.map(function (h, i) {
    var b = Buffer.from(h, 'hex');
    if (asStrings) { return b.toString('latin1'); }               // (ASCII patterns only)
    return i % 2 ? new Uint8Array(b) : b;
  });
}

var job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
var rep = { cases: [] };
job.cases.forEach(function (c) {
  var input = fs.readFileSync(c.path);
  var index = Bzip2.buildIndex(input, c.multistream);
  var target = c.damaged ? fs.readFileSync(c.damaged) : input;
  var patterns = unhex(c.patterns, c.asStrings);
  rep.cases.push(attempt(function () { return Bzip2.searchRegex(target, index, patterns, c.opts); }));
  if (!rep.refusals) {
    var refuse = function (p) { return attempt(function () { return Bzip2.searchRegex(input, index, ['fine', p], {}); }); };
    rep.refusals = {
      none: attempt(function () { return Bzip2.searchRegex(input, index, [], {}); }),
      empty: refuse(''),
      anchor: refuse('a$'),
      boundary: refuse('\\bfoo'),
      lazy: refuse('a*?'),
      matchesEmpty: refuse('a*'),
      paren: refuse('(ab'),
      bound: refuse('a{257}'),
      states: refuse('(a|b)*a(a|b){8}'),
      long: refuse(Buffer.alloc(1025, 97)),
      fraction: attempt(function () { return Bzip2.searchRegex(input, index, ['a'], { offset: 1.5 }); }),
      notAnIndex: attempt(function () { return Bzip2.searchRegex(input, new Uint8Array(40), ['a']); }),
      check: attempt(function () { return Bzip2.regexCheck(['ok', '[a'], { nocase: true }); })
    };
  }
});
rep.check = attempt(function () { return Bzip2.regexCheck(unhex(job.check, false)); });
rep.checkNocase = attempt(function () { return Bzip2.regexCheck(unhex(job.check, true), { nocase: true }); });
console.log(JSON.stringify(rep));
