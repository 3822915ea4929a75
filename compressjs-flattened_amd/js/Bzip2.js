'use strict';
/* Bzip2.js — drop-in front for the reference's `Bzip2` object (J/Bzip2_joined_.js:2198-2253):
 * same method names, argument meaning and error behaviour; the per-block pipeline runs in
 * libcjs_hip.so on an MI355X through the N-API addon.  No JavaScript fallback. */
var common = require('./common.js');

var Err = { OK: 0, LAST_BLOCK: -1, NOT_BZIP_DATA: -2, UNEXPECTED_INPUT_EOF: -3, UNEXPECTED_OUTPUT_EOF: -4,
            DATA_ERROR: -5, OUT_OF_MEMORY: -6, OBSOLETE_INPUT: -7, END_OF_BLOCK: -8 };
var Messages = {};
Messages[Err.NOT_BZIP_DATA] = 'Not bzip data';
Messages[Err.DATA_ERROR] = 'Data error';
Messages[Err.OUT_OF_MEMORY] = 'Out of memory';
Messages[Err.OBSOLETE_INPUT] = 'Obsolete (pre 0.9.5) bzip format not supported.';

function rethrow(e) {
  if (e && typeof e.cjsCode === 'number') {
    var code = e.cjsCode;
    if (code === -20) { throw new Error('Invalid block size multiplier'); }      // J/Bzip2_joined_.js:2208
    if (Messages[code]) {                                                       // _throw(status, optDetail) :1385-1391
      var msg = Messages[code];
      if (e.cjsDetail) { msg += ': ' + e.cjsDetail; }
      var t = new TypeError(msg); t.errorCode = code; throw t;
    }
    var g = new Error(e.message); g.errorCode = code; throw g;
  }
  throw e;
}

// A stream object in the reference's sense (Util.coerceInputStream / coerceOutputStream): it has the byte method and no backing
// buffer of its own (a Buffer, a typed array and a plain array are not streams).
function isStream(x, method) {
  return x !== null && typeof x === 'object' && method in x && !(x instanceof Uint8Array) && !Array.isArray(x);
}
var IN_PIECE = 4 << 20, OUT_PIECE = 4 << 20, FEED_PIECE = 64 << 10;
// Output budget of the decoder behind decompressFile and cli.js -d: a quarter of the library's default.  The decoder's device
// scratch is proportional to it (~2 GB at 64 MiB for a level-9 stream, held even for a small file), and a front has no caller
// who could size it.
var FRONT_OUT_BYTES = 64 << 20;
// up to buf.length bytes of the stream into buf; 0 at its end
function fillFrom(inStream, buf) {
  if (typeof inStream.read === 'function') { var got = inStream.read(buf, 0, buf.length); return got > 0 ? got : 0; }
  var n = 0, ch;
  while (n < buf.length && (ch = inStream.readByte()) !== -1 && ch !== undefined && ch >= 0) { buf[n++] = ch; }
  return n;
}
function writeTo(outStream, piece) {
  if (typeof outStream.write === 'function') { outStream.write(piece, 0, piece.length); return; }
  for (var i = 0; i < piece.length; i++) { outStream.writeByte(piece[i]); }
}
// compressFile with a stream object on either side: the input is fed to the streaming encoder piece by piece and the output is
// drained as it appears; neither the whole input nor (with an output stream) the whole result is ever held.  tables (optional,
// compressFileIndexed): {lines}; the encoder keeps the stream's block index (and line table), left in tables.index / .lineIndex.
function compressPiecewise(inStream, inIsStream, outStream, outIsStream, level, tables) {
  var a = common.addon(), enc = null, pieces = [], total = 0;
  function drain() {
    while (a.bzip2EncPending(enc) > 0) {
      var p = a.bzip2EncRead(enc, OUT_PIECE);
      if (outIsStream) { writeTo(outStream, p); } else { pieces.push(p); total += p.length; }
    }
  }
  try {
    enc = tables ? a.bzip2EncCreate(level, 0, tables.lines ? 12 : 4) : a.bzip2EncCreate(level, 0);      // CJS_FLAG_ENC_INDEX | _LINES
    if (inIsStream) {
      var buf = new Uint8Array(IN_PIECE), n;
      while ((n = fillFrom(inStream, buf)) > 0) { a.bzip2EncWrite(enc, buf.subarray(0, n)); drain(); }
    } else {
      var bytes = common.coerceInput(inStream).bytes;
      for (var off = 0; off < bytes.length; off += IN_PIECE) { a.bzip2EncWrite(enc, bytes.subarray(off, Math.min(bytes.length, off + IN_PIECE))); drain(); }
    }
    a.bzip2EncFinish(enc);
    drain();
    if (tables) { var t = a.bzip2EncIndex(enc, !!tables.lines); tables.index = t.index; tables.lineIndex = t.lineIndex; }
  } catch (e) { rethrow(e); } finally { if (enc) { a.bzip2EncDestroy(enc); } }
  if (outIsStream) {
    if (outStream.flush) { outStream.flush(); }
    return outStream;
  }
  var result = new Uint8Array(total), o = 0;
  pieces.forEach(function (p) { result.set(p, o); o += p.length; });
  return common.deliver(result, outStream);
}

// decompressFile with a stream object on either side: the .bz2 stream is fed to the streaming decoder piece by piece and the
// decoded bytes are drained as they appear (a pull model: the decoder takes what its window has room for, reading runs the GPU
// steps).  A stream that fails throws the reference's error once every block in front of the failure has reached the sink.
function decompressPiecewise(inStream, inIsStream, outStream, outIsStream, multistream) {
  var a = common.addon(), dec = null, pieces = [], total = 0, obuf = new Uint8Array(OUT_PIECE);
  function drain() {
    var got;
    while ((got = a.bzip2DecRead(dec, obuf)) > 0) {
      if (outIsStream) { writeTo(outStream, obuf.subarray(0, got)); } else { pieces.push(obuf.slice(0, got)); total += got; }
    }
  }
  // Fed in pieces of the smallest chunk the decoder can have, with a drain behind each: a step then runs as soon as chunk_bytes
  // wait, whatever the chunk is, and the output never lags the input by more than that.  A short write means the window is full:
  // after a drain the next one takes at least a byte.
  function feed(piece) {
    while (piece.length > 0) {
      var part = piece.subarray(0, Math.min(piece.length, FEED_PIECE));
      piece = piece.subarray(a.bzip2DecWrite(dec, part));
      drain();
    }
  }
  try {
    dec = a.bzip2DecCreate(multistream ? 1 : 0, 0, FRONT_OUT_BYTES);
    if (inIsStream) {
      var buf = new Uint8Array(IN_PIECE), n;
      while ((n = fillFrom(inStream, buf)) > 0) { feed(buf.subarray(0, n)); }
    } else {
      var bytes = common.coerceInput(inStream).bytes;
      for (var off = 0; off < bytes.length; off += IN_PIECE) { feed(bytes.subarray(off, Math.min(bytes.length, off + IN_PIECE))); }
    }
    a.bzip2DecFinish(dec);
    drain();
  } catch (e) { rethrow(e); } finally { if (dec) { a.bzip2DecDestroy(dec); } }
  if (outIsStream) {
    if (outStream.flush) { outStream.flush(); }
    return outStream;
  }
  var result = new Uint8Array(total), o = 0;
  pieces.forEach(function (p) { result.set(p, o); o += p.length; });
  return common.deliver(result, outStream);
}

var Bzip2 = Object.create(null);
Bzip2.compressFile = function (inStream, outStream, props) {
  var level = 9;
  if (typeof props === 'number') { level = props; }
  if (level < 1 || level > 9) { throw new Error('Invalid block size multiplier'); }
  var inIsStream = isStream(inStream, 'readByte'), outIsStream = isStream(outStream, 'writeByte');
  if (inIsStream || outIsStream) { return compressPiecewise(inStream, inIsStream, outStream, outIsStream, level); }
  var input = common.coerceInput(inStream);
  var result;
  try { result = common.addon().bzip2Compress(input.bytes, level); } catch (e) { rethrow(e); }
  return common.deliver(result, outStream);
};
// compressFile that also hands out the tables of its stream (cjs_bzip2_compress_indexed, cjs_bzip2_enc_index): returns {output:
// what compressFile returns, index: what buildIndex(output) returns, lineIndex: what buildLineIndex(output, index) returns, or
// null with opts.lines === false}, without the table pass and the full decode those two take.  With a stream object on either
// side the streaming encoder keeps the tables (36 bytes per block) while the stream passes through.  opts: {lines = true}.
Bzip2.compressFileIndexed = function (inStream, outStream, props, opts) {
  var level = 9, lines = !(opts && opts.lines === false);
  if (typeof props === 'number') { level = props; }
  if (level < 1 || level > 9) { throw new Error('Invalid block size multiplier'); }
  var inIsStream = isStream(inStream, 'readByte'), outIsStream = isStream(outStream, 'writeByte');
  if (inIsStream || outIsStream) {
    var tables = { lines: lines, index: null, lineIndex: null };
    var output = compressPiecewise(inStream, inIsStream, outStream, outIsStream, level, tables);
    return { output: output, index: tables.index, lineIndex: tables.lineIndex };
  }
  var input = common.coerceInput(inStream);
  var r;
  try { r = common.addon().bzip2CompressIndexed(input.bytes, level, lines); } catch (e) { rethrow(e); }
  return { output: common.deliver(r.data, outStream), index: r.index, lineIndex: r.lineIndex };
};
// Bzip2.compressFile over a batch: one stream per input, in input order, all inputs in one pass per stage on the GPU
Bzip2.compressFiles = function (inStreams, props) {
  var level = 9;
  if (typeof props === 'number') { level = props; }
  if (level < 1 || level > 9) { throw new Error('Invalid block size multiplier'); }
  var inputs = [];
  for (var i = 0; i < inStreams.length; i++) { inputs.push(common.coerceInput(inStreams[i]).bytes); }
  try { return common.addon().bzip2CompressBatch(inputs, level); } catch (e) { rethrow(e); }
};
Bzip2.decompressFile = function (inStream, outStream, multistream) {
  var inIsStream = isStream(inStream, 'readByte'), outIsStream = isStream(outStream, 'writeByte');
  if (inIsStream || outIsStream) { return decompressPiecewise(inStream, inIsStream, outStream, outIsStream, multistream); }
  var input = common.coerceInput(inStream);
  var result;
  try { result = common.addon().bzip2Decompress(input.bytes, multistream ? 1 : 0); } catch (e) { rethrow(e); }
  return common.deliver(result, outStream);
};
// Bzip2.decompressFile over a batch: one output per input, in input order, decoded in shared GPU passes.  If an input fails,
// the error decompressFile would throw for the lowest-index failing one, with e.index = its index.
Bzip2.decompressFiles = function (inStreams, multistream) {
  var inputs = [];
  for (var i = 0; i < inStreams.length; i++) { inputs.push(common.coerceInput(inStreams[i]).bytes); }
  try { return common.addon().bzip2DecompressBatch(inputs, multistream ? 1 : 0); } catch (e) {
    try { rethrow(e); } catch (t) { if (typeof e.cjsIndex === 'number') { t.index = e.cjsIndex; } throw t; }
  }
};
// Bunzip.decodeBlock (J/Bzip2_joined_.js:1797-1818): the block whose magic starts at bit `pos`
Bzip2.decompressBlock = function (inStream, pos, outStream) {
  var input = common.coerceInput(inStream);
  var result;
  try { result = common.addon().bzip2DecompressBlock(input.bytes, pos); } catch (e) { rethrow(e); }
  return common.deliver(result, outStream);
};
// Bunzip.table (:1823-1863): callback(position in bits, uncompressed size in bytes) once per block
Bzip2.table = function (inStream, callback, multistream) {
  var input = common.coerceInput(inStream);
  var t;
  try { t = common.addon().bzip2Table(input.bytes, multistream ? 1 : 0); } catch (e) { rethrow(e); }
  for (var i = 0; i < t.length; i += 2) { callback(t[i], t[i + 1]); }
};
// What bzip2recover is for (cjs_bzip2_recover): the intact blocks of damaged .bz2 data -- any bytes, no header needed -- as their
// decoded bytes, or with asStream as a repaired single-stream .bz2.  callback(position in bits, uncompressed size in bytes,
// status) once per block magic in the input, ascending: status 0 = recovered, Bzip2.REC_SHADOWED = a false magic inside a
// recovered block, else the block's error code (size 0 then).  The bytes are delivered like decompressFile's.
Bzip2.recoverFile = function (inStream, outStream, callback, asStream) {
  var input = common.coerceInput(inStream);
  var r;
  try { r = common.addon().bzip2Recover(input.bytes, asStream ? 1 : 0); } catch (e) { rethrow(e); }
  if (typeof callback === 'function') {
    for (var i = 0; i < r.found.length; i += 6) { callback(r.found[i], r.found[i + 3], r.found[i + 4]); }
  }
  return common.deliver(r.data, outStream);
};
// Indexed range reads (cjs_bzip2_read_ranges): bytes [offset, offset + length) of what decompressFile(input, null, multistream)
// returns, decoding only the blocks they touch.  buildIndex makes the block index of a stream in its serialised form (a
// Uint8Array to keep beside the file); readRange and readRanges take it back.  A range is clipped at the end of the data, like
// pread.  readRanges(input, index, [[offset, length], ...]) returns one entry per range: its bytes, or -- for a range that touches
// a block that is damaged or does not agree with the index -- the TypeError readRange throws for it (the detail on the
// lowest-index one).
Bzip2.buildIndex = function (inStream, multistream) {
  var input = common.coerceInput(inStream);
  try { return common.addon().bzip2BuildIndex(input.bytes, multistream ? 1 : 0); } catch (e) { rethrow(e); }
};
Bzip2.readRanges = function (inStream, index, ranges) {
  var input = common.coerceInput(inStream), flat = new Float64Array(2 * ranges.length), r;
  for (var i = 0; i < ranges.length; i++) { flat[2 * i] = ranges[i][0]; flat[2 * i + 1] = ranges[i][1]; }
  try { r = common.addon().bzip2ReadRanges(input.bytes, index, flat); } catch (e) { rethrow(e); }
  var out = [], detail = r.detail;
  for (var k = 0; k < ranges.length; k++) {
    var code = r.layout[3 * k + 2];
    if (code === 0) { out.push(r.data.subarray(r.layout[3 * k], r.layout[3 * k] + r.layout[3 * k + 1])); continue; }
    var t = new TypeError((Messages[code] || 'Data error') + (detail ? ': ' + detail : ''));
    t.errorCode = code; detail = '';
    out.push(t);
  }
  return out;
};
Bzip2.readRange = function (inStream, index, offset, length) {
  var r = Bzip2.readRanges(inStream, index, [[offset, length]])[0];
  if (r instanceof Error) { throw r; }
  return r;
};
// Pattern search (cjs_bzip2_search): where `patterns` (strings, Buffers or Uint8Arrays; 1..64 of 1..256 bytes) occur in bytes
// [offset, offset + length) of the decoded data, found on the GPU; only the matches come back.  opts: {offset = 0, length = to the
// end, nocase = false (ASCII letters only), limit = every match}.  Returns {matches: [[offset, pattern], ...] sorted by (offset,
// pattern), total: all matches of the window, badBlocks, firstBadBlock (null if none), detail}: a damaged block does not fail
// the search, nothing matches across it.
Bzip2.search = function (inStream, index, patterns, opts) {
  var input = common.coerceInput(inStream), o = opts || {}, parts = [], lens = new Float64Array(patterns.length), r;
  for (var i = 0; i < patterns.length; i++) {
    var b = typeof patterns[i] === 'string' ? Buffer.from(patterns[i], 'utf8') : Buffer.from(common.coerceInput(patterns[i]).bytes);
    parts.push(b); lens[i] = b.length;
  }
  try {
    r = common.addon().bzip2Search(input.bytes, index, new Uint8Array(Buffer.concat(parts)), lens, o.nocase ? 1 : 0, o.offset === undefined ? 0 : o.offset,
                                   o.length === undefined || o.length === null ? -1 : o.length, o.limit === undefined || o.limit === null ? -1 : o.limit);
  } catch (e) { rethrow(e); }
  var matches = [];
  for (var k = 0; k < r.matches.length; k += 2) { matches.push([r.matches[k], r.matches[k + 1]]); }
  return { matches: matches, total: r.total, badBlocks: r.badBlocks, firstBadBlock: r.firstBadBlock < 0 ? null : r.firstBadBlock, detail: r.detail };
};
// Regex search (cjs_bzip2_search_regex): Bzip2.search with patterns that are bounded regular expressions (strings, Buffers or
// Uint8Arrays of 1..1024 bytes; the dialect and the clamp at 256 bytes are described in cjs_hip.h).  Same opts and result, the
// matches [[offset, pattern, length], ...], length the longest match at that offset.  A pattern the dialect refuses throws an Error
// whose message ends in the library's detail ("pattern J, byte P: ...") and whose errorCode is the library's code.
function patternBytes(patterns) {
  var parts = [], lens = new Float64Array(patterns.length);
  for (var i = 0; i < patterns.length; i++) {
    var b = typeof patterns[i] === 'string' ? Buffer.from(patterns[i], 'utf8') : Buffer.from(common.coerceInput(patterns[i]).bytes);
    parts.push(b); lens[i] = b.length;
  }
  return { bytes: new Uint8Array(Buffer.concat(parts)), lens: lens };
}
function rethrowWithDetail(e) {
  if (e && typeof e.cjsCode === 'number' && !Messages[e.cjsCode] && e.cjsDetail) {
    var g = new Error(e.message + ': ' + e.cjsDetail); g.errorCode = e.cjsCode; throw g;
  }
  rethrow(e);
}
Bzip2.searchRegex = function (inStream, index, patterns, opts) {
  var input = common.coerceInput(inStream), o = opts || {}, p = patternBytes(patterns), r;
  try {
    r = common.addon().bzip2SearchRegex(input.bytes, index, p.bytes, p.lens, o.nocase ? 1 : 0, o.offset === undefined ? 0 : o.offset,
                                        o.length === undefined || o.length === null ? -1 : o.length, o.limit === undefined || o.limit === null ? -1 : o.limit);
  } catch (e) { rethrowWithDetail(e); }
  var matches = [];
  for (var k = 0; k < r.matches.length; k += 3) { matches.push([r.matches[k], r.matches[k + 1], r.matches[k + 2]]); }
  return { matches: matches, total: r.total, badBlocks: r.badBlocks, firstBadBlock: r.firstBadBlock < 0 ? null : r.firstBadBlock, detail: r.detail };
};
// Compile only, without a device (cjs_regex_check): [{states, maxLen}, ...] per pattern; opts: {nocase = false}.
Bzip2.regexCheck = function (patterns, opts) {
  var p = patternBytes(patterns), r, out = [];
  try { r = common.addon().regexCheck(p.bytes, p.lens, opts && opts.nocase ? 1 : 0); } catch (e) { rethrowWithDetail(e); }
  for (var k = 0; k < r.length; k += 2) { out.push({ states: r[k], maxLen: r[k + 1] }); }
  return out;
};
// Compare (cjs_bzip2_compare, cjs_bzip2_compare_streams): `cmp` / `bzcmp` on the GPU; only the differing bytes come back.
// compare: byte k of `other` (plain bytes) against decoded byte otherOffset + k, inside [offset, offset + length).  compareStreams:
// the decoded bytes of stream A against those of stream B.  opts: {offset = 0, length = to the end, otherOffset = 0, limit = 64
// (null: every difference)}.  Returns {equal, diffs: [{offset, a, b}, ...] ascending (a: the stream's byte, b: the other side's),
// total: all differences of the span, firstDiff (null if none), compared: the bytes actually compared, lenA, lenB: where the two
// sides end, badBlocks, firstBadBlock, badBlocksB, firstBadBlockB (null if none), detail}: a damaged block does not fail the
// compare, its bytes are not compared.  equal: no difference, no bad block, both sides of one length and compared whole.
function compareResult(r) {
  var diffs = [];
  for (var k = 0; k < r.diffs.length; k += 3) { diffs.push({ offset: r.diffs[k], a: r.diffs[k + 1], b: r.diffs[k + 2] }); }
  return { equal: r.total === 0 && r.badBlocks === 0 && r.badBlocksB === 0 && r.lenA === r.lenB && r.compared === r.lenA,
           diffs: diffs, total: r.total, firstDiff: r.firstDiff < 0 ? null : r.firstDiff, compared: r.compared, lenA: r.lenA, lenB: r.lenB,
           badBlocks: r.badBlocks, firstBadBlock: r.firstBadBlock < 0 ? null : r.firstBadBlock, badBlocksB: r.badBlocksB,
           firstBadBlockB: r.firstBadBlockB < 0 ? null : r.firstBadBlockB, detail: r.detail };
}
function compareCall(input, index, other, otherIndex, o) {
  try {
    return compareResult(common.addon().bzip2Compare(input.bytes, index, other.bytes, otherIndex, o.otherOffset === undefined ? 0 : o.otherOffset,
                                                     o.offset === undefined ? 0 : o.offset, o.length === undefined || o.length === null ? -1 : o.length,
                                                     o.limit === undefined ? 64 : o.limit === null ? -1 : o.limit));
  } catch (e) { rethrow(e); }
}
Bzip2.compare = function (inStream, index, other, opts) {
  return compareCall(common.coerceInput(inStream), index, common.coerceInput(other), null, opts || {});
};
Bzip2.compareStreams = function (inStreamA, indexA, inStreamB, indexB, opts) {
  var o = opts || {};
  return compareCall(common.coerceInput(inStreamA), indexA, common.coerceInput(inStreamB), indexB, { offset: o.offset, length: o.length, limit: o.limit });
};
// The line table (cjs_bzip2_lines_*): lines are numbered from 0 and end with their '\n' (0x0A, nothing else); line N, behind the
// last newline, is the unterminated tail.  buildLineIndex counts the newlines of every block on the GPU and returns the table in
// its serialised form (a Uint8Array to keep beside the index).  lineStarts gives the decoded offset where each line starts (the
// end of the data for a line past the last), lineNumbers the line each decoded offset belongs to; both decode at most one block
// per question and return {values: [...], status: [...], detail}: status is 0 or the code of a question whose block is damaged
// (its value is 0 then).  readLines returns lines first .. first + count - 1 as bytes, by one lineStarts and one readRange.
Bzip2.buildLineIndex = function (inStream, index) {
  var input = common.coerceInput(inStream);
  try { return common.addon().bzip2BuildLineIndex(input.bytes, index); } catch (e) { rethrow(e); }
};
function linesAsk(inStream, index, lineIndex, questions, kind) {
  var input = common.coerceInput(inStream), r;
  try { r = common.addon().bzip2LinesAsk(input.bytes, index, lineIndex, Float64Array.from(questions), kind); } catch (e) { rethrow(e); }
  return { values: Array.from(r.answers), status: Array.from(r.status), detail: r.detail };
}
Bzip2.lineStarts = function (inStream, index, lineIndex, lines) { return linesAsk(inStream, index, lineIndex, lines, 0); };
Bzip2.lineNumbers = function (inStream, index, lineIndex, offsets) { return linesAsk(inStream, index, lineIndex, offsets, 1); };
Bzip2.readLines = function (inStream, index, lineIndex, first, count) {
  var at = Bzip2.lineStarts(inStream, index, lineIndex, [first, first + count]);
  for (var k = 0; k < 2; k++) {
    if (at.status[k] !== 0) {
      var t = new TypeError((Messages[at.status[k]] || 'Data error') + (at.detail ? ': ' + at.detail : ''));
      t.errorCode = at.status[k];
      throw t;
    }
  }
  return Bzip2.readRange(inStream, index, at.values[0], at.values[1] - at.values[0]);
};
// The line keys (cjs_bzip2_line_keys): a 16-byte record per line, hashed on the GPU while the blocks stand decoded there.  lineKeys
// returns {keys: Uint8Array (16 bytes per line, little-endian: u64 hash, u32 len, u32 check; all ones: the line touches a damaged
// block), lines, badBlocks, firstBadBlock (null if none), detail} for lines first .. first + count - 1 (count undefined: to the
// last).  Equal records mean equal lines up to a hash collision; the hash's bases follow from seed alone, so against crafted
// input pass a seed of your own.  diffLines is bzdiff: the keys of both streams, then the line diff on the host: {hunks: [{aFirst,
// aCount, bFirst, bCount}] ascending, edits, common, minimal}; an empty final line is dropped from either side first, as diff does;
// a damaged block on either side throws.  maxEdits (0: 16,384): above it the middle is one hunk and minimal is false.
function lineKeysCall(inStream, index, lineIndex, o) {
  var input = common.coerceInput(inStream), r;
  try {
    r = common.addon().bzip2LineKeys(input.bytes, index, lineIndex, o.first === undefined ? 0 : o.first, o.count === undefined || o.count === null ? -1 : o.count,
                                     o.seed === undefined ? 0 : o.seed);
  } catch (e) { rethrow(e); }
  return { keys: r.keys, lines: r.lines, badBlocks: r.badBlocks, firstBadBlock: r.firstBadBlock < 0 ? null : r.firstBadBlock, detail: r.detail };
}
Bzip2.lineKeys = function (inStream, index, lineIndex, opts) { return lineKeysCall(inStream, index, lineIndex, opts || {}); };
Bzip2.diffLines = function (inStreamA, indexA, lineIndexA, inStreamB, indexB, lineIndexB, opts) {
  var o = opts || {}, sides = [[inStreamA, indexA, lineIndexA], [inStreamB, indexB, lineIndexB]].map(function (s) {
    var r = lineKeysCall(s[0], s[1], s[2], { seed: o.seed });
    if (r.badBlocks) {
      var t = new TypeError(Messages[Err.DATA_ERROR] + (r.detail ? ': ' + r.detail : '')); t.errorCode = Err.DATA_ERROR; throw t;
    }
    var k = r.keys, last = k.length - 16, empty = true;
    for (var i = last; i < k.length; i++) { empty = empty && k[i] === 0; }
    return empty ? k.subarray(0, last) : k;
  });
  var d;
  try { d = common.addon().lineKeysDiff(sides[0], sides[1], o.maxEdits === undefined ? 0 : o.maxEdits); } catch (e) { rethrow(e); }
  var hunks = [];
  for (var j = 0; j < d.hunks.length; j += 4) { hunks.push({ aFirst: d.hunks[j], aCount: d.hunks[j + 1], bFirst: d.hunks[j + 2], bCount: d.hunks[j + 3] }); }
  return { hunks: hunks, edits: d.edits, common: d.common, minimal: d.minimal };
};
// The column cut (cjs_bzip2_cut): `bzcat | cut -f LIST -d D` / `cut -b LIST`, selected and packed on the GPU; only the selected bytes
// come back, as a Buffer.  opts: {fields | bytes (exactly one): a cut-style string ("1,3-5,7-") or an array of numbers and [lo, hi]
// pairs (hi null: to the end of the line); delimiter = '\t' (one byte: a string, a Buffer or a number); first = 0, count = to the
// last line}.  A line without the delimiter is a line of one field (GNU cut prints it whole).  A damaged block inside the window
// throws; every error carries errorCode and ends in the library's detail.
function cutList(spec) {
  if (typeof spec === 'string') { return spec; }
  var flat = [];
  for (var i = 0; i < spec.length; i++) {
    if (Array.isArray(spec[i])) { flat.push(spec[i][0], spec[i][1] === null || spec[i][1] === undefined ? -1 : spec[i][1]); } else { flat.push(spec[i], spec[i]); }
  }
  return Float64Array.from(flat);
}
function cutDelimiter(d) {
  if (d === undefined) { d = '\t'; }
  if (typeof d === 'number') { return d; }
  var raw = typeof d === 'string' ? Buffer.from(d, 'latin1') : Buffer.from(common.coerceInput(d).bytes);
  if (raw.length !== 1) { throw new TypeError('the delimiter is one byte'); }
  return raw[0];
}
Bzip2.cutLines = function (inStream, index, lineIndex, opts) {
  var input = common.coerceInput(inStream), o = opts || {}, r;
  if ((o.fields === undefined || o.fields === null) === (o.bytes === undefined || o.bytes === null)) { throw new TypeError('exactly one of fields and bytes must be given'); }
  var byBytes = o.fields === undefined || o.fields === null, d = cutDelimiter(o.delimiter);
  try {
    r = common.addon().bzip2Cut(input.bytes, index, lineIndex, byBytes ? 1 : 0, d, cutList(byBytes ? o.bytes : o.fields), o.first === undefined ? 0 : o.first,
                                o.count === undefined || o.count === null ? -1 : o.count);
  } catch (e) { rethrowWithDetail(e); }
  return Buffer.from(r.buffer, r.byteOffset, r.length);
};
// The line frequency table (cjs_bzip2_tally; `bzcat | sort | uniq -c | sort -rn | head`): the lines' keys are made and grouped on the
// GPU and only the groups come down.  tallyLines returns {groups: Uint8Array (32 bytes per group, little-endian: u64 hash, u32 len,
// u32 check, u64 first = the number of the group's first line, u64 count), nLines, nDistinct, nGroups, nBadLines, maxCount,
// badBlocks, firstBadBlock (null if none), detail} for lines first .. first + count - 1 (count undefined: to the last).  order
// 'count' (default): descending count, ties by first occurrence; 'first': by first occurrence.  minCount 2 is uniq -d, maxCount 1 is
// uniq -u; limit: the first so many groups (undefined: all).  A tail without a newline counts as the line with one; lines that touch
// a damaged block are counted in nBadLines and grouped nowhere.  fields | bytes (with delimiter, as cutLines takes them): the tally
// of that cut -- which values of a column occur how often; a damaged block inside the window then throws as it does in cutLines.
Bzip2.tallyLines = function (inStream, index, lineIndex, opts) {
  var o = opts || {}, input = common.coerceInput(inStream), r;
  var order = o.order === undefined || o.order === 'count' ? 1 : o.order === 'first' ? 0 : -1;
  if (order < 0) throw new TypeError("order is 'count' or 'first'");
  var noFields = o.fields === undefined || o.fields === null, noBytes = o.bytes === undefined || o.bytes === null;
  if (!noFields && !noBytes) { throw new TypeError('at most one of fields and bytes may be given'); }
  var mode = noFields && noBytes ? 2 : noFields ? 1 : 0;
  try {
    r = common.addon().bzip2Tally(input.bytes, index, lineIndex, o.first === undefined ? 0 : o.first, o.count === undefined || o.count === null ? -1 : o.count,
                                  o.seed === undefined ? 0 : o.seed, order, o.minCount === undefined ? 1 : o.minCount, o.maxCount === undefined ? 0 : o.maxCount,
                                  o.limit === undefined || o.limit === null ? -1 : o.limit, mode, mode === 2 ? 0 : cutDelimiter(o.delimiter),
                                  mode === 2 ? '' : cutList(mode === 1 ? o.bytes : o.fields));
  } catch (e) { rethrowWithDetail(e); }
  r.firstBadBlock = r.firstBadBlock < 0 ? null : r.firstBadBlock;
  return r;
};
// The line sort (cjs_bzip2_sort; `bzcat | sort`, `| sort | head`, `| sort -u`, `| cut .. | sort`): the lines are ordered by content on
// the GPU and only their numbers come down.  sortLines returns {lines: Float64Array of line numbers in LC_ALL=C order of their content
// (equal lines by ascending number), counts: Float64Array (the size of each entry's run of equal lines; all ones without unique),
// text: Buffer of the returned entries' lines, each with a newline (only with text: true), nLines, nOut, nDistinct, textBytes, rounds}
// for lines first .. first + count - 1 (count undefined: to the last).  reverse: descending content, equal lines still ascending;
// unique: one entry per run of equal lines, its lowest number; limit: the first so many entries (undefined: all).  fields | bytes
// (with delimiter, as cutLines takes them): the cut of each line is what is compared and what text holds; the numbers stay those of
// whole lines.  A damaged block inside the window throws as it does in cutLines.
Bzip2.sortLines = function (inStream, index, lineIndex, opts) {
  var o = opts || {}, input = common.coerceInput(inStream), r;
  var noFields = o.fields === undefined || o.fields === null, noBytes = o.bytes === undefined || o.bytes === null;
  if (!noFields && !noBytes) { throw new TypeError('at most one of fields and bytes may be given'); }
  var mode = noFields && noBytes ? 2 : noFields ? 1 : 0;
  try {
    r = common.addon().bzip2Sort(input.bytes, index, lineIndex, o.first === undefined ? 0 : o.first, o.count === undefined || o.count === null ? -1 : o.count,
                                 (o.reverse ? 1 : 0) | (o.unique ? 2 : 0), o.limit === undefined || o.limit === null ? -1 : o.limit, !!o.text, mode,
                                 mode === 2 ? 0 : cutDelimiter(o.delimiter), mode === 2 ? '' : cutList(mode === 1 ? o.bytes : o.fields));
  } catch (e) { rethrowWithDetail(e); }
  if (r.text !== undefined) { r.text = Buffer.from(r.text.buffer, r.text.byteOffset, r.text.length); }
  return r;
};
Bzip2.REC_SHADOWED = 1;
Bzip2.Err = Err;
module.exports = Bzip2;
