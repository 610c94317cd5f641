// Host-side mirror of the reference's src/parallel.ts for the MI355X engine.
//
//   import { Weierstraß, TwistedEdwards, startThreads, stopThreads } from "./parallel.mjs";
//   await startThreads();
//   const Curve = await Weierstraß.create(bls12377Params);
//   let [pointPtr] = await Curve.Parallel.randomPointsFast(N);
//   let [scalarPtr] = await Curve.Parallel.randomScalars(N);
//   let { result, log } = await Curve.Parallel.msmUnsafe(scalarPtr, pointPtr, N, true);
//   Curve.Projective.toAffine(scratch, affPtr, result); Curve.Affine.toBigint(affPtr)  // or toBigint(result)
//
// Same names / argument order / promise-returning style as parallel.ts:149-158, 263-271.  The
// reference's "pointers" into wasm memory become opaque handles to GPU-resident arrays; all the
// arithmetic happens in HIP behind the N-API addon (napi/msmz_napi.c -> include/msmz.h).  This file is
// plain ECMAScript (valid TypeScript; declarations in parallel.d.ts) so that it runs without a
// compile step on the image's node 12.
import { createRequire } from "module";
import { dirname, join } from "path";
import { fileURLToPath } from "url";

const require = createRequire(import.meta.url);
const here = dirname(fileURLToPath(import.meta.url));
let addon = null;
function native() {
  // fails loudly if the addon / libmsmz.so has not been built: there is no wasm or JS fallback
  if (addon === null) addon = require(join(here, "msmz_napi.node"));
  return addon;
}

let devices = null;

/** parallel.ts:291-315.  The reference spawns n-1 workers that share one MSM; here the workers are GPUs: a curve
 * created after startThreads(n) drives GPUs first..first+n-1 (inputs split over them, partial sums added on the
 * host: msmz_create with n_devices = n).  Without n: one GPU, LOCAL_RANK or 0.  `deviceId` may also be an array
 * of ids. */
export async function startThreads(n, deviceId) {
  if (Array.isArray(deviceId)) devices = deviceId.map(Number);
  else {
    const first = deviceId !== undefined ? Number(deviceId) : n === undefined || n === 1 ? Number(process.env.LOCAL_RANK || 0) : 0;
    devices = Array.from({ length: n || 1 }, (_, i) => first + i);
  }
  if (devices.length < 1 || devices.length > 8) throw Error(`startThreads: 1..8 GPUs, got ${devices.length}`);
  native();
  return devices.length === 1 ? devices[0] : devices;
}

/** parallel.ts:317-320 */
export async function stopThreads() {
  devices = null;
}

function bytesToBigint(buf, off, len) {
  let x = 0n;
  for (let i = len - 1; i >= 0; i--) x = (x << 8n) | BigInt(buf[off + i]);
  return x;
}
function bigintToBytes(x, len) {
  const out = Buffer.alloc(len);
  for (let i = 0; i < len; i++) {
    out[i] = Number(x & 0xffn);
    x >>= 8n;
  }
  return out;
}

/** a scalar as the addon takes it: 32 bytes, little-endian */
const scalarBuf = (v) => Buffer.from(bigintToBytes(v, 32));

/** the range checks of every operation over resident arrays: ranges = [[name, first, array or null], ...] -> n (absent:
 * what the shortest array leaves).  Every `first` is an index of its array, and 0 without one; 1 <= n < limit fits every
 * array from its `first`.  With `out` the last range is the destination: it may be an input's range exactly or apart
 * from it, never overlap it in part. */
function scanRanges(who, ranges, n, out = null, limit = 2 ** 32) {
  for (const [name, first, arr] of ranges) {
    if (!Number.isInteger(first) || first < 0 || (arr === null ? first !== 0 : first >= arr.n))
      throw Error(`${who}: ${name} = ${first}` + (arr === null ? " without the array it indexes" : ` but the array holds ${arr.n}`));
  }
  if ((n === undefined || n === null) && ranges.some((r) => r[2] !== null))
    n = Math.min(...ranges.filter((r) => r[2] !== null).map(([, first, arr]) => arr.n - first));
  if (!Number.isInteger(n) || n < 1 || n >= limit) throw Error(`${who}: n = ${n}`);
  for (const [name, first, arr] of ranges)
    if (arr !== null && n > arr.n - first) throw Error(`${who}: entries [${first}, +${n}) from ${name} of an array of ${arr.n}`);
  const firstOut = ranges[ranges.length - 1][1];
  if (out !== null)
    for (const [name, first, arr] of ranges.slice(0, -1))
      if (arr !== null && arr.handle === out.handle && first !== firstOut && Math.abs(first - firstOut) < n)
        throw Error(`${who}: the destination [${firstOut}, +${n}) overlaps the input range [${first}, +${n}) (${name}) in part`);
  return n;
}

/** The arguments of Parallel.ntt -> {logN, flags, nIn, count, first, firstOut, root, shift}, checked before anything
 * reaches the device (msm_zprize_amd/parallel.py ntt_args is the same function).  root / shift: a bigint or null.  Whether
 * `root` is a primitive root of unity, and whether the field has transforms of this length, is the library's to say. */
/** compressed / sign of pointsFromBytes and pointsToCompressedBytes, checked before any call -> {compressed, sign} */
export function compressedArgs(who, compressed = false, sign = "largest", montgomery = false) {
  if (typeof compressed !== "boolean") throw TypeError(`${who}: compressed is true or false`);
  if (sign !== "largest" && sign !== "parity") throw Error(`${who}: sign is "largest" or "parity", got ${String(sign)}`);
  if (!compressed && sign !== "largest") throw Error(`${who}: sign "parity" describes compressed records (compressed: true)`);
  if (compressed && montgomery) throw Error(`${who}: compressed records are canonical, not Montgomery residues`);
  return { compressed, sign };
}

export function nttArgs(x, logN, { inverse = false, shift = null, root = null, nIn = null, count = 1, first = 0, out = null, firstOut = 0 } = {}, order) {
  const who = "ntt";
  // (anything with the three fields of a resident array will do here: Parallel.ntt asks for the real thing first)
  const isScalars = (v) => v !== null && typeof v === "object" && v.kind === "scalars" && Number.isInteger(v.n) && v.handle !== undefined;
  if (!isScalars(x)) throw TypeError(`${who}: \`x\` is a resident scalar array`);
  if (out !== null && !isScalars(out)) throw TypeError(`${who}: \`out\` is a resident scalar array or null`);
  if (typeof inverse !== "boolean") throw TypeError(`${who}: \`inverse\` is a boolean`);
  for (const [name, v] of [["shift", shift], ["root", root]]) {
    if (v !== null && typeof v !== "bigint") throw TypeError(`${who}: \`${name}\` is a bigint or null`);
    if (v !== null && (v < 0n || v >= order)) throw Error(`${who}: ${name} = ${v} is not in [0, group order)`);
  }
  if (shift === 0n) throw Error(`${who}: the coset shift is not 0`);
  if (!Number.isInteger(logN) || logN < 0 || logN >= 32) throw Error(`${who}: logN = ${logN} (0..31)`);
  const n = 2 ** logN;
  if (!Number.isInteger(count) || count < 1 || count * n >= 2 ** 32)
    throw Error(`${who}: count = ${count} transforms of ${n} entries (1 <= count, count * n < 2^32)`);
  if (nIn === null) nIn = n;
  if (!Number.isInteger(nIn) || nIn < 1 || nIn > n) throw Error(`${who}: nIn = ${nIn} (1..${n})`);
  if (inverse && nIn !== n) throw Error(`${who}: an inverse transform reads whole vectors (nIn = ${nIn}, n = ${n})`);
  for (const [name, v, arr] of [["first", first, x], ["firstOut", firstOut, out]]) {
    if (!Number.isInteger(v) || v < 0) throw Error(`${who}: ${name} = ${v}`);
    if (arr === null && v !== 0) throw Error(`${who}: ${name} = ${v} without the array it indexes`);
  }
  if (count * nIn > x.n - first) throw Error(`${who}: entries [${first}, +${count * nIn}) of an array of ${x.n}`);
  if (out !== null) {
    if (count * n > out.n - firstOut) throw Error(`${who}: entries [${firstOut}, +${count * n}) of an array of ${out.n}`);
    const same = first === firstOut && nIn === n;
    const apart = first + count * nIn <= firstOut || firstOut + count * n <= first;
    if (out.handle === x.handle && !same && !apart)
      throw Error(`${who}: the destination [${firstOut}, +${count * n}) overlaps the source [${first}, +${count * nIn}) in part`);
  }
  return { logN, flags: (inverse ? 1 : 0) | (shift !== null ? 2 : 0), nIn, count, first, firstOut, root, shift };
}

/** the limits of the multilinear calls (include/msmz.h) */
export const MLE_MAX_VARS = 31, SUMCHECK_MAX_TABLES = 6, SUMCHECK_MAX_DEGREE = 4, SUMCHECK_MAX_TERMS = 8;
const looksLikeScalars = (v) => v !== null && typeof v === "object" && v.kind === "scalars" && Number.isInteger(v.n) && v.handle !== undefined;

/** a point of a multilinear polynomial: an array of at most 31 bigints below the group order -> its number of variables */
function mlePoint(who, point, order) {
  if (!Array.isArray(point) || !point.every((r) => typeof r === "bigint")) throw TypeError(`${who}: \`point\` is an array of bigints, one per variable`);
  if (point.length > MLE_MAX_VARS) throw Error(`${who}: ${point.length} variables (at most ${MLE_MAX_VARS})`);
  point.forEach((r, j) => {
    if (r < 0n || r >= order) throw Error(`${who}: point[${j}] = ${r} is not in [0, group order)`);
  });
  return point.length;
}
const mleFirst = (who, name, first, arr) => {
  if (!Number.isInteger(first) || first < 0) throw Error(`${who}: ${name} = ${first}`);
  if (arr === null && first !== 0) throw Error(`${who}: ${name} = ${first} without the array it indexes`);
};
function mleVars(who, nVars, have, what) {
  if (nVars === null || nVars === undefined) {
    if (have < 2 || 2 ** Math.round(Math.log2(have)) !== have) throw Error(`${who}: nVars is needed: ${what} ${have} entries, not a power of two >= 2`);
    return Math.round(Math.log2(have));
  }
  if (!Number.isInteger(nVars) || nVars < 1 || nVars > MLE_MAX_VARS) throw Error(`${who}: nVars = ${nVars} (1..${MLE_MAX_VARS})`);
  return nVars;
}

/** The arguments of Parallel.eqTable -> {nVars, scale}, of Parallel.evaluateMle -> {nVars, first}, of Parallel.bindMle ->
 * {nVars, count, flags, first, firstOut, n} and of Parallel.sumcheckRound -> {tables, nVars, terms, flags, degree}, checked
 * before anything reaches the device (msm_zprize_amd/parallel.py eq_table_args, mle_eval_args, mle_bind_args and
 * sumcheck_round_args are the same functions). */
export function eqTableArgs(point, scale, order) {
  const nVars = mlePoint("eqTable", point, order);
  if (typeof scale !== "bigint") throw TypeError("eqTable: `scale` is a bigint");
  if (scale < 0n || scale >= order) throw Error(`eqTable: scale = ${scale} is not in [0, group order)`);
  return { nVars, scale: scale === 1n ? null : scale };
}
export function mleEvalArgs(f, point, { first = 0 } = {}, order) {
  const who = "evaluateMle";
  if (!looksLikeScalars(f)) throw TypeError(`${who}: \`f\` is a resident scalar array`);
  const nVars = mlePoint(who, point, order);
  mleFirst(who, "first", first, f);
  if (2 ** nVars > f.n - first) throw Error(`${who}: entries [${first}, +${2 ** nVars}) of an array of ${f.n}`);
  return { nVars, first };
}
export function mleBindArgs(f, r, { nVars = null, count = 1, low = false, first = 0, out = null, firstOut = 0 } = {}, order) {
  const who = "bindMle";
  if (!looksLikeScalars(f)) throw TypeError(`${who}: \`f\` is a resident scalar array`);
  if (out !== null && !looksLikeScalars(out)) throw TypeError(`${who}: \`out\` is a resident scalar array or null`);
  if (typeof r !== "bigint") throw TypeError(`${who}: \`r\` is a bigint`);
  if (typeof low !== "boolean") throw TypeError(`${who}: \`low\` is a boolean`);
  if (r < 0n || r >= order) throw Error(`${who}: r = ${r} is not in [0, group order)`);
  if (!Number.isInteger(count) || count < 1) throw Error(`${who}: count = ${count}`);
  mleFirst(who, "first", first, f);
  mleFirst(who, "firstOut", firstOut, out);
  const have = f.n - first;
  if (nVars === null && (have < 0 || have % count !== 0)) throw Error(`${who}: nVars is needed: ${have} entries are not ${count} equal tables`);
  nVars = mleVars(who, nVars, nVars === null ? have / count : 0, "a table would hold");
  const n = 2 ** nVars, h = n / 2;
  if (count * n >= 2 ** 32) throw Error(`${who}: count = ${count} tables of ${n} entries (count * 2^nVars < 2^32)`);
  if (count * n > have) throw Error(`${who}: entries [${first}, +${count * n}) of an array of ${f.n}`);
  if (out !== null) {
    if (count * h > out.n - firstOut) throw Error(`${who}: entries [${firstOut}, +${count * h}) of an array of ${out.n}`);
    const inPlace = count === 1 && !low && firstOut === first;
    const apart = firstOut + count * h <= first || first + count * n <= firstOut;
    if (out.handle === f.handle && !inPlace && !apart)
      throw Error(`${who}: the destination [${firstOut}, +${count * h}) overlaps the source [${first}, +${count * n}); it may be the low half of ONE table bound in its high variable, or apart from the source`);
  }
  return { nVars, count, flags: low ? 1 : 0, first, firstOut, n: count * h };
}
export function sumcheckRoundArgs(tables, terms, { nVars = null, low = false } = {}, order, who = "sumcheckRound") {
  if (!Array.isArray(tables) || !Array.isArray(terms)) throw TypeError(`${who}: \`tables\` and \`terms\` are arrays`);
  if (typeof low !== "boolean") throw TypeError(`${who}: \`low\` is a boolean`);
  const tabs = tables.map((t) => {
    // (a resident array IS an Array of one element, itself: a pair is a plain array of two)
    const [arr, first] = Array.isArray(t) && !looksLikeScalars(t) && t.length === 2 ? t : [t, 0];
    if (!looksLikeScalars(arr)) throw TypeError(`${who}: a table is a resident scalar array or an [array, first] pair`);
    mleFirst(who, "first", first, arr);
    return [arr, first];
  });
  if (tabs.length < 1 || tabs.length > SUMCHECK_MAX_TABLES) throw Error(`${who}: ${tabs.length} tables (1..${SUMCHECK_MAX_TABLES})`);
  if (terms.length < 1 || terms.length > SUMCHECK_MAX_TERMS) throw Error(`${who}: ${terms.length} terms (1..${SUMCHECK_MAX_TERMS})`);
  let degree = 0;
  const out = terms.map((t) => {
    if (!Array.isArray(t) || t.length !== 2) throw TypeError(`${who}: a term is a pair [coefficient, mask]`);
    const [c, mask] = t;
    if (c !== null && typeof c !== "bigint") throw TypeError(`${who}: a coefficient is a bigint or null (1)`);
    if (!Number.isInteger(mask)) throw TypeError(`${who}: a mask is an integer, bit j for table j`);
    if (c !== null && (c < 0n || c >= order)) throw Error(`${who}: the coefficient ${c} is not in [0, group order)`);
    let factors = 0;
    for (let m = mask; m > 0; m = Math.floor(m / 2)) factors += m % 2;
    if (mask <= 0 || mask >= 2 ** tabs.length || factors > SUMCHECK_MAX_DEGREE)
      throw Error(`${who}: mask = ${mask}: 1..${SUMCHECK_MAX_DEGREE} of the ${tabs.length} tables`);
    degree = Math.max(degree, factors);
    return [c, mask];
  });
  nVars = mleVars(who, nVars, tabs[0][0].n - tabs[0][1], "the first table holds");
  for (const [arr, first] of tabs)
    if (2 ** nVars > arr.n - first) throw Error(`${who}: entries [${first}, +${2 ** nVars}) of an array of ${arr.n}`);
  return { tables: tabs, nVars, terms: out, flags: low ? 1 : 0, degree };
}

/** The arguments of Parallel.sumcheckStep -> {tables, out, nVars, terms, flags, degree}: those of sumcheckRound, then r,
 * then the destinations and the overlap rules of include/msmz.h, checked before anything reaches the device
 * (msm_zprize_amd/parallel.py sumcheck_step_args is the same function).  out: [[array, first]] or null (every table in
 * place); degree: that of the polynomial returned (0 when nVars is 1). */
export function sumcheckStepArgs(tables, terms, r, { nVars = null, out = null, low = false } = {}, order, who = "sumcheckStep") {
  const t = sumcheckRoundArgs(tables, terms, { nVars, low }, order, who);
  if (typeof r !== "bigint") throw TypeError(`${who}: \`r\` is a bigint`);
  if (out !== null && !Array.isArray(out)) throw TypeError(`${who}: \`out\` is an array with one destination per table, or null`);
  const outs = (out || []).map((o) => {
    const [arr, first] = Array.isArray(o) && !looksLikeScalars(o) && o.length === 2 ? o : [o, 0];
    if (!looksLikeScalars(arr)) throw TypeError(`${who}: a destination is a resident scalar array or an [array, first] pair`);
    mleFirst(who, "first", first, arr);
    return [arr, first];
  });
  if (r < 0n || r >= order) throw Error(`${who}: r = ${r} is not in [0, group order)`);
  const tabs = t.tables, n = 2 ** t.nVars, h = n / 2;
  if (out !== null && outs.length !== tabs.length) throw Error(`${who}: ${outs.length} destinations for ${tabs.length} tables`);
  const dst = out === null ? tabs : outs;
  for (const [arr, first] of outs)
    if (h > arr.n - first) throw Error(`${who}: entries [${first}, +${h}) of an array of ${arr.n}`);
  const meet = (a, fa, na, b, fb, nb) => a.handle === b.handle && fa < fb + nb && fb < fa + na;
  dst.forEach(([d, df], j) => {
    for (let k = 0; k < j; k++)
      if (meet(d, df, h, dst[k][0], dst[k][1], h)) throw Error(`${who}: the destinations of tables ${k} and ${j} overlap`);
    tabs.forEach(([s, sf], k) => {
      if (!meet(d, df, h, s, sf, n)) return;
      if (k !== j) throw Error(`${who}: the destination of table ${j} overlaps table ${k}`);
      if (low || df !== sf)
        throw Error(`${who}: the destination of table ${j} overlaps its table; it may be the table's low half [${sf}, +${h}) with low = false, or apart from it`);
    });
  });
  return { ...t, out: out === null ? null : outs, degree: t.nVars > 1 ? t.degree : 0 };
}

/** The arguments of Parallel.innerProducts -> {rows, cols ([[array, first]]), n, firstOut}, checked before anything reaches
 * the device, in the order of msmz_scalars_dot_many (include/msmz.h): the types, the two counts, n, firstOut without an
 * array, every range inside its array, and a destination range that meets no input range
 * (msm_zprize_amd/parallel.py inner_products_args is the same function). */
export const DOT_MANY_MAX_ROWS = 128, DOT_MANY_MAX_COLS = 8;
export function dotManyArgs(rows, cols, n = null, { out = null, firstOut = 0 } = {}, who = "innerProducts") {
  const vectors = (vs, name) => {
    if (!Array.isArray(vs)) throw TypeError(`${who}: \`${name}\` is an array of resident scalar arrays or [array, first] pairs`);
    return vs.map((v) => {
      const [arr, first] = Array.isArray(v) && v.length === 2 ? v : [v, 0];
      if (!looksLikeScalars(arr) || !Number.isInteger(first))
        throw TypeError(`${who}: a vector of \`${name}\` is a resident scalar array or an [array, first] pair`);
      return [arr, first];
    });
  };
  const rv = vectors(rows, "rows"), cv = vectors(cols, "cols");
  if (out !== null && !looksLikeScalars(out)) throw TypeError(`${who}: \`out\` is a resident scalar array or null`);
  if (n !== null && !Number.isInteger(n)) throw TypeError(`${who}: \`n\` is an integer or null`);
  if (!Number.isInteger(firstOut)) throw TypeError(`${who}: \`firstOut\` is an integer`);
  if (rv.length < 1 || rv.length > DOT_MANY_MAX_ROWS) throw Error(`${who}: ${rv.length} rows (1 to ${DOT_MANY_MAX_ROWS})`);
  if (cv.length < 1 || cv.length > DOT_MANY_MAX_COLS) throw Error(`${who}: ${cv.length} columns (1 to ${DOT_MANY_MAX_COLS})`);
  const all = [...rv, ...cv];
  for (const [arr, first] of all) if (first < 0 || first > arr.n) throw Error(`${who}: first = ${first} of an array of ${arr.n}`);
  if (n === null) n = Math.min(...all.map(([arr, first]) => arr.n - first));
  if (n < 1 || n >= 2 ** 32) throw Error(`${who}: n = ${n}`);
  if (firstOut < 0 || (out === null && firstOut !== 0)) throw Error(`${who}: firstOut = ${firstOut}${out === null ? " without the array it indexes" : ""}`);
  for (const [arr, first] of all) if (n > arr.n - first) throw Error(`${who}: entries [${first}, +${n}) of an array of ${arr.n}`);
  if (out !== null) {
    const results = rv.length * cv.length;
    if (firstOut > out.n || results > out.n - firstOut) throw Error(`${who}: entries [${firstOut}, +${results}) of an array of ${out.n}`);
    for (const [arr, first] of all)
      if (arr.handle === out.handle && first < firstOut + results && firstOut < first + n)
        throw Error(`${who}: the destination [${firstOut}, +${results}) meets the input range [${first}, +${n}) of the same array`);
  }
  return { rows: rv, cols: cv, n, firstOut };
}

/** The arguments of Parallel.sparseMatrix -> {rows, cols (Buffers of little-endian u32), nnz, shape, flags, firstValue} and
 * of Parallel.matVec -> {n, flags}, checked before anything reaches the device (msm_zprize_amd/parallel.py
 * sparse_matrix_args and mat_vec_args are the same functions).  `values` here is a resident scalar array or null: a host
 * list is uploaded by the caller first. */
const ORIENTATIONS = { rows: 1, cols: 2, both: 3 };
function indexBuffer(who, name, v, bound) {
  if (!(Array.isArray(v) || v instanceof Uint32Array)) throw TypeError(`${who}: \`${name}\` is an array of integers or a Uint32Array`);
  const buf = Buffer.alloc(4 * v.length);
  for (let k = 0; k < v.length; k++) {
    if (!Number.isInteger(v[k])) throw TypeError(`${who}: \`${name}\` is an array of integers or a Uint32Array`);
    if (v[k] < 0 || v[k] >= bound) throw Error(`${who}: ${name}[${k}] = ${v[k]} is not in [0, ${bound})`);
    buf.writeUInt32LE(v[k], 4 * k);
  }
  return buf;
}
export function sparseMatrixArgs(rows, cols, values, { shape = null, orientations = "rows", firstValue = 0 } = {}) {
  const who = "sparseMatrix";
  if (!Array.isArray(shape) || shape.length !== 2 || !shape.every(Number.isInteger)) throw TypeError(`${who}: \`shape\` is a pair of integers [nRows, nCols]`);
  if (!Object.prototype.hasOwnProperty.call(ORIENTATIONS, orientations)) throw Error(`${who}: orientations = ${orientations} ("rows", "cols" or "both")`);
  const [nRows, nCols] = shape;
  if (nRows < 1 || nRows >= 2 ** 32) throw Error(`${who}: nRows = ${nRows}`);
  if (nCols < 1 || nCols >= 2 ** 32) throw Error(`${who}: nCols = ${nCols}`);
  if (values !== null && !looksLikeScalars(values)) throw TypeError(`${who}: \`values\` is a resident scalar array, an array of bigints or null`);
  const r = indexBuffer(who, "rows", rows, nRows), c = indexBuffer(who, "cols", cols, nCols);
  const nnz = rows.length;
  if (cols.length !== nnz) throw Error(`${who}: ${nnz} rows but ${cols.length} cols`);
  if (nnz < 1 || nnz >= 2 ** 32) throw Error(`${who}: N = ${nnz}`);
  mleFirst(who, "firstValue", firstValue, values);
  if (values !== null && nnz > values.n - firstValue) throw Error(`${who}: entries [${firstValue}, +${nnz}) from firstValue of an array of ${values.n}`);
  return { rows: r, cols: c, nnz, shape: [nRows, nCols], flags: ORIENTATIONS[orientations], firstValue };
}
const looksLikeMatrix = (m) => m !== null && typeof m === "object" && m.kind === "matrix" && Array.isArray(m.shape) && typeof m.orientations === "string";
export function matVecArgs(matrix, x, { firstX = 0, transpose = false, out = null, firstOut = 0 } = {}) {
  const who = "matVec";
  if (!looksLikeMatrix(matrix)) throw TypeError(`${who}: \`matrix\` is a sparse matrix (sparseMatrix)`);
  if (!looksLikeScalars(x)) throw TypeError(`${who}: \`x\` is a resident scalar array`);
  if (out !== null && !looksLikeScalars(out)) throw TypeError(`${who}: \`out\` is a resident scalar array or null`);
  if (typeof transpose !== "boolean") throw TypeError(`${who}: \`transpose\` is a boolean`);
  if (matrix.handle === null) throw Error(`${who}: the matrix was freed`);
  const need = transpose ? "cols" : "rows";
  if (matrix.orientations !== need && matrix.orientations !== "both")
    throw Error(`${who}: transpose=${transpose} needs a matrix built with orientations "${need}" or "both", this one has "${matrix.orientations}"`);
  const [nOut, nIn] = transpose ? [matrix.shape[1], matrix.shape[0]] : matrix.shape;
  mleFirst(who, "firstX", firstX, x);
  mleFirst(who, "firstOut", firstOut, out);
  if (nIn > x.n - firstX) throw Error(`${who}: entries [${firstX}, +${nIn}) from firstX of an array of ${x.n}`);
  if (out !== null) {
    if (nOut > out.n - firstOut) throw Error(`${who}: entries [${firstOut}, +${nOut}) from firstOut of an array of ${out.n}`);
    if (out.handle === x.handle && firstOut < firstX + nIn && firstX < firstOut + nOut)
      throw Error(`${who}: the destination [${firstOut}, +${nOut}) overlaps the input range [${firstX}, +${nIn}) (firstX); x is gathered, so the two may not meet at all`);
  }
  return { n: nOut, flags: transpose ? 1 : 0 };
}

/** The arguments of Parallel.lookupMultiplicities -> {n, tableN}, checked before anything reaches the device
 * (msm_zprize_amd/parallel.py lookup_args is the same function).  n: the column entries looked up; tableN: the table
 * entries, which is also the entries written. */
export function lookupArgs(column, table, { firstColumn = 0, n = null, firstTable = 0, tableN = null, out = null, firstOut = 0, positions = false } = {}) {
  const who = "lookupMultiplicities";
  if (!looksLikeScalars(column)) throw TypeError(`${who}: \`column\` is a resident scalar array`);
  if (!looksLikeScalars(table)) throw TypeError(`${who}: \`table\` is a resident scalar array`);
  if (out !== null && !looksLikeScalars(out)) throw TypeError(`${who}: \`out\` is a resident scalar array or null`);
  if (typeof positions !== "boolean") throw TypeError(`${who}: \`positions\` is a boolean`);
  mleFirst(who, "firstColumn", firstColumn, column);
  mleFirst(who, "firstTable", firstTable, table);
  mleFirst(who, "firstOut", firstOut, out);
  const size = (name, v, first, arr, limit) => {
    const k = v === null ? arr.n - first : v;
    if (!Number.isInteger(k) || k < 1 || k > limit) throw Error(`${who}: ${name} = ${k}`);
    if (k > arr.n - first) throw Error(`${who}: entries [${first}, +${k}) of an array of ${arr.n} (${name})`);
    return k;
  };
  const N = size("n", n, firstColumn, column, 2 ** 32 - 1), T = size("tableN", tableN, firstTable, table, 2 ** 30);
  if (out !== null) {
    if (T > out.n - firstOut) throw Error(`${who}: entries [${firstOut}, +${T}) from firstOut of an array of ${out.n}`);
    for (const [name, arr, first, len] of [["table", table, firstTable, T], ["column", column, firstColumn, N]])
      if (out.handle === arr.handle && firstOut < first + len && first < firstOut + T)
        throw Error(`${who}: the destination [${firstOut}, +${T}) overlaps the ${name} range [${first}, +${len}); both inputs are gathered, so it may meet neither at all`);
  }
  return { n: N, tableN: T };
}

/** The arguments of Parallel.evaluateExpression -> {columns: [[array, first]], terms: [[bigint | null, [[column, rot]]]], n},
 * checked before anything reaches the device (msm_zprize_amd/parallel.py expr_args is the same function). */
export const EXPR_MAX_COLUMNS = 16, EXPR_MAX_TERMS = 32, EXPR_MAX_DEGREE = 8, EXPR_MAX_OPERANDS = 32;
export function exprArgs(columns, terms, { n = null, out = null, firstOut = 0 } = {}, order) {
  const who = "evaluateExpression";
  if (!Array.isArray(columns) || looksLikeScalars(columns) || !Array.isArray(terms)) throw TypeError(`${who}: \`columns\` and \`terms\` are arrays`);
  if (out !== null && !looksLikeScalars(out)) throw TypeError(`${who}: \`out\` is a resident scalar array or null`);
  const cols = columns.map((c) => {
    // (a resident array IS an Array of one element, itself: a pair is a plain array of two)
    const [arr, first] = Array.isArray(c) && !looksLikeScalars(c) && c.length === 2 ? c : [c, 0];
    if (!looksLikeScalars(arr)) throw TypeError(`${who}: a column is a resident scalar array or an [array, first] pair`);
    return [arr, first];
  });
  if (cols.length < 1 || cols.length > EXPR_MAX_COLUMNS) throw Error(`${who}: ${cols.length} columns (1..${EXPR_MAX_COLUMNS})`);
  if (terms.length < 1 || terms.length > EXPR_MAX_TERMS) throw Error(`${who}: ${terms.length} terms (1..${EXPR_MAX_TERMS})`);
  const parsed = terms.map((t) => {
    if (!Array.isArray(t) || t.length !== 2 || !Array.isArray(t[1])) throw TypeError(`${who}: a term is a pair [coefficient, [factors]]`);
    const [c, factors] = t;
    if (c !== null && typeof c !== "bigint") throw TypeError(`${who}: a coefficient is a bigint or null (1)`);
    if (c !== null && (c < 0n || c >= order)) throw Error(`${who}: the coefficient ${c} is not in [0, group order)`);
    const fs = factors.map((f) => {
      const [col, rot] = Array.isArray(f) && f.length === 2 ? f : [f, 0];
      if (!Number.isInteger(col) || !Number.isInteger(rot)) throw TypeError(`${who}: a factor is a column index or a pair [column, rot] of integers`);
      if (col < 0 || col >= cols.length) throw Error(`${who}: a factor names column ${col} of ${cols.length}`);
      if (rot < -(2 ** 31) || rot >= 2 ** 31) throw Error(`${who}: rot = ${rot} is no int32`);
      return [col, rot];
    });
    if (fs.length > EXPR_MAX_DEGREE) throw Error(`${who}: a term of ${fs.length} factors (0..${EXPR_MAX_DEGREE})`);
    return [c, fs];
  });
  cols.forEach(([arr, first], k) => {
    mleFirst(who, `the first of column ${k}`, first, arr);
    if (first >= arr.n) throw Error(`${who}: the first of column ${k} = ${first} but the array holds ${arr.n}`);
  });
  mleFirst(who, "firstOut", firstOut, out);
  if (out !== null && firstOut >= out.n) throw Error(`${who}: firstOut = ${firstOut} but the array holds ${out.n}`);
  if (n === null) {
    const lengths = [...new Set(cols.map(([arr, first]) => arr.n - first))].sort((a, b) => a - b);
    if (lengths.length !== 1) throw Error(`${who}: N is needed when the columns hold different numbers of entries: ${lengths}`);
    n = lengths[0];
  }
  if (!Number.isInteger(n) || n < 1 || n >= 2 ** 32) throw Error(`${who}: N = ${n}`);
  cols.forEach(([arr, first], k) => {
    if (n > arr.n - first) throw Error(`${who}: entries [${first}, +${n}) from the first of column ${k} of an array of ${arr.n}`);
  });
  if (out !== null && n > out.n - firstOut) throw Error(`${who}: entries [${firstOut}, +${n}) from firstOut of an array of ${out.n}`);
  const mod = (rot) => ((rot % n) + n) % n;
  const operands = new Set();
  for (const [, fs] of parsed) for (const [col, rot] of fs) operands.add(`${col}:${mod(rot)}`);
  if (operands.size > EXPR_MAX_OPERANDS)
    throw Error(`${who}: the terms read ${operands.size} distinct (column, rot mod N) pairs (at most ${EXPR_MAX_OPERANDS})`);
  if (out !== null)
    cols.forEach(([arr, first], k) => {
      const rots = [...operands].filter((o) => o.startsWith(`${k}:`)).map((o) => Number(o.split(":")[1]));
      if (arr.handle !== out.handle || rots.length === 0) return;
      if (rots.every((r) => r === 0)) {
        if (first !== firstOut && Math.abs(first - firstOut) < n)
          throw Error(`${who}: the destination [${firstOut}, +${n}) overlaps the input range [${first}, +${n}) (column ${k}) in part; it may be that range exactly or apart from it`);
      } else if (Math.abs(first - firstOut) < n) {
        throw Error(`${who}: the destination [${firstOut}, +${n}) overlaps the input range [${first}, +${n}) (column ${k}); the column is read rotated, so the two may not meet at all`);
      }
    });
  return { columns: cols, terms: parsed, n };
}

/** A GPU-resident sparse matrix (msmz_matrix_create): shape = [rows, columns], nnz, the orientations it was built for */
class SparseMatrix {
  constructor(curve, handle, shape, nnz, orientations) {
    Object.assign(this, { curve, handle, shape, nnz, orientations, kind: "matrix" });
  }
  free() {
    if (this.handle !== null) native().free(this.curve._ctx, this.handle);
    this.handle = null;
  }
}

/** A GPU-resident input array; destructures like the reference's pointer arrays: `let [ptr] = ...` */
class DeviceArray extends Array {
  static make(curve, handle, n, kind) {
    const a = new DeviceArray();
    a.push(a);
    Object.defineProperties(a, {
      curve: { value: curve }, handle: { value: handle, writable: true }, n: { value: n }, kind: { value: kind },
    });
    return a;
  }
  free() {
    if (this.handle !== null) native().free(this.curve._ctx, this.handle);
    this.handle = null;
  }
}
const isScalars = (v) => v instanceof DeviceArray && v.kind === "scalars";
const isPoints = (v) => v instanceof DeviceArray && v.kind === "points";

// ---------------------------------------------------------------------------------------------------------------
// Pointer-style routes of the reference (src/parallel.ts:89-133, src/curve-affine.ts:290-308, Scalar.writeBigint):
//   let pointPtr = await Parallel.getPointer(nMax * Affine.size);          // parallel.ts:89-91
//   Field.memoryBytes.set(bytes, pointInputPtr);                           // host bytes -> "wasm memory"
//   await Parallel.pointsFromBytes(pointPtr, pointInputPtr, n);            // parallel.ts:97-112
//   Affine.writeBigints(pointPtr, points); Scalar.writeBigint(scalarPtr + i * Scalar.sizeField, s);
//   await Parallel.msmUnsafe(scalarPtr, pointPtr, n);
// The reference's pointers are byte offsets into wasm memory and its scripts do arithmetic on them, so the shims
// keep them NUMBERS: addresses in a virtual space, each region backed by a host staging buffer and (once an MSM or
// a conversion needs it) a GPU-resident array.  Record sizes are this engine's wire sizes (Affine.size = 2 fe_bytes,
// Scalar.sizeField = 32), not the wasm limb sizes; scripts that use the named constants need no other change.
class Region {
  constructor(base, size, kind) {
    this.base = base; this.size = size; this.kind = kind;   // kind: "field" | "scalar"
    this.host = null;      // Buffer of staged records (canonical little-endian bytes)
    this.inf = null;       // Uint8Array of infinity flags (points written with isZero)
    this.count = 0;        // records staged
    this.dirty = false;    // host bytes newer than the device copy
    this.device = null;    // DeviceArray
  }
}
const REGION_ALIGN = 2 ** 20;
function makePointerSpace() {
  const regions = [];
  let next = REGION_ALIGN;   // 0 stays the null pointer
  return {
    alloc(size, kind) {
      const r = new Region(next, size, kind);
      regions.push(r);
      next += Math.ceil((size + 1) / REGION_ALIGN) * REGION_ALIGN;
      return r.base;
    },
    find(ptr) {   // -> [region, byte offset]
      for (const r of regions) if (ptr >= r.base && ptr < r.base + Math.max(r.size, 1)) return [r, ptr - r.base];
      throw Error(`pointer ${ptr} was not returned by getPointer / getScalarPointer`);
    },
  };
}

function createCurve(params, kind) {
  if (params.kind !== kind) throw Error(`${params.label} is not a ${kind} curve`);
  if (devices === null) devices = [Number(process.env.LOCAL_RANK || 0)];
  const N = native();
  const ctx = N.create(params.curveId, devices.length === 1 ? devices[0] : devices);
  const fb = params.feBytes;
  const te = kind === "twisted-edwards";
  const curve = { params, _ctx: ctx };
  const space = makePointerSpace();
  const recSize = { field: 2 * fb, scalar: 32 };
  function stage(region, offset, bytes, count) {   // copy `bytes` into the region's host buffer at byte offset
    if (offset + bytes.length > region.size) throw Error("write beyond the end of the pointer's allocation");   // memory-helpers.ts:224-236
    if (region.host === null) region.host = Buffer.alloc(region.size);
    Buffer.from(bytes.buffer, bytes.byteOffset, bytes.length).copy(region.host, offset);
    region.count = Math.max(region.count, count);
    region.dirty = true;
  }
  // the GPU-resident array behind a pointer (uploaded on first use / after the staged bytes changed)
  function resident(ptr, n, what) {
    if (ptr instanceof DeviceArray) return ptr;
    const [r, off] = space.find(ptr);
    if (off !== 0) throw Error(`${what}: an MSM input must start at the pointer getPointer returned`);
    if (r.dirty || r.device === null || r.device.n < n) {
      if (r.host === null || r.count < n) throw Error(`${what}: ${r.count} records were written, ${n} needed`);
      if (r.device) r.device.free();
      const size = recSize[r.kind];
      const bytes = r.host.subarray(0, r.count * size);
      r.device = r.kind === "scalar"
        ? DeviceArray.make(curve, N.uploadScalars(ctx, bytes, r.count), r.count, "scalars")
        : DeviceArray.make(curve, N.uploadPoints(ctx, bytes, r.inf && r.inf.some((v) => v) ? Buffer.from(r.inf.subarray(0, r.count)) : null, r.count), r.count, "points");
      r.dirty = false;
    }
    return r.device;
  }

  function decodePoint(buf, off, isInf) {
    const p = { x: bytesToBigint(buf, off, fb), y: bytesToBigint(buf, off + fb, fb) };
    if (!te) {
      p.isZero = !!isInf;
      if (p.isZero) { p.x = 0n; p.y = 1n; } // bigint/projective-weierstrass.ts:210
    }
    return p;
  }

  function decodePoints(r, count) {   // the {xy, isInf} of the addon's msmBatch / msmSegments -> count results
    return Array.from({ length: count }, (_, k) => decodePoint(r.xy, 2 * fb * k, r.isInf[k]));
  }

  // options.scalarBits: "every scalar of this call is below 2^scalarBits" (msmz_opts.reserved[1]); 0 / absent = no bound.
  // Checked here, before anything reaches the device.
  function scalarBitsArg(options, who) {
    const bits = options.scalarBits;
    if (bits === undefined || bits === null) return 0;
    if (!Number.isInteger(bits) || bits < 0 || bits > 256) throw Error(`${who}: scalarBits = ${bits} (0 = no bound, or 1..256)`);
    return bits;
  }

  // the options of an MSM call as the addon takes them; buckets undefined: options.buckets
  function msmOpts(options, who, safe, buckets, timing = 0) {
    return {
      c: options.c || 0,
      glv: options.glv !== undefined ? Number(options.glv) : te ? 0 : -1,   // -1: GLV below 2^21 points (include/msmz.h)
      safe: options.useSafeAdditions !== undefined ? Number(options.useSafeAdditions) : safe,
      buckets: buckets === undefined ? options.buckets || 0 : buckets,
      timing,
      reduceAffine: options.reduceAffine ? 1 : 0, // batched-affine first reduction level (reduceBucketsAffine)
      scalarBits: scalarBitsArg(options, who),
    };
  }

  // the pointer form (ptr, inputPtr, n) of pointsFromBytes / scalarsFromBytes: the bytes were put behind inputPtr with
  // memoryBytes.set, the converted (Montgomery, GPU-resident) records end up behind ptr.  Range errors (a coordinate >= p)
  // surface here, like every upload.
  function fromPointer(who, ptr, inputPtr, count, size, upload, kind) {
    const [dst, doff] = space.find(ptr), [src, soff] = space.find(inputPtr);
    if (doff !== 0 || src.host === null || soff + count * size > src.size) throw Error(`${who}(ptr, inputPtr, n): bad pointers`);
    if (dst.device) dst.device.free();
    const bytes = src.host.subarray(soff, soff + count * size);
    dst.device = DeviceArray.make(curve, upload(bytes), count, kind);
    dst.host = bytes; dst.count = count; dst.dirty = false; dst.inf = null;
  }

  async function msmCommon(scalars, points, n, verbose, options, safe, buckets) {
    const opts = msmOpts(options || {}, "msm", safe, buckets, verbose ? 1 : 0);
    if (typeof points === "number") points = resident(points, n, "msm points");
    if (typeof scalars === "number") scalars = resident(scalars, n, "msm scalars");
    const s = scalars instanceof DeviceArray ? scalars.handle : scalars; // Buffer = host scalars
    const r = N.msm(ctx, points.handle, s, n, fb, opts);
    const result = decodePoint(r.xy, 0, r.isInf);
    const log = [[{ n: Math.ceil(Math.log2(n)), K: r.log.K, c: r.log.c }]];
    for (const [k, v] of Object.entries(r.log.stageMs)) log.push([`${k}... ${v.toFixed(3)}ms`]);
    return { result, log, stats: r.log };
  }

  // B MSMs over the first n points in one device pipeline (msmz_msm_batch): `scalarsList` is ONE resident scalar array
  // of >= B * n scalars (vector k = entries [k n, (k + 1) n); B = options.batch, default length / n) or an array of B
  // host byte arrays (scalarsFromBytes format, concatenated here).  A list of resident arrays is refused.
  async function msmBatchCommon(scalarsList, points, n, options, safe) {
    options = options || {};
    const opts = msmOpts(options, "msmBatch", safe);
    if (typeof points === "number") points = resident(points, n, "msmBatch points");
    if (!(n > 0) || n > points.n) throw Error(`msmBatch: n = ${n} but the point set holds ${points.n}`);
    let s, B;
    if (scalarsList instanceof DeviceArray) {
      B = options.batch !== undefined ? Number(options.batch) : Math.floor(scalarsList.n / n);
      if (!(B > 0) || B * n > scalarsList.n) throw Error(`msmBatch: ${B} vectors of ${n} scalars, the array holds ${scalarsList.n}`);
      s = scalarsList.handle;
    } else {
      if (!Array.isArray(scalarsList) || scalarsList.length === 0) throw Error("msmBatch: one resident scalar array or a list of host byte arrays");
      if (scalarsList.some((v) => v instanceof DeviceArray || typeof v === "number"))
        throw Error("msmBatch: a list of resident arrays is not accepted; pass ONE resident array of B * n scalars");
      const len = scalarsList[0].length;
      if (scalarsList.some((v) => v.length !== len)) throw Error("msmBatch: scalar vectors of unequal length");
      if (len < 32 * n) throw Error(`msmBatch: a vector of ${len} bytes holds fewer than n = ${n} scalars`);
      B = scalarsList.length;
      s = Buffer.concat(scalarsList.map((v) => Buffer.from(v.buffer, v.byteOffset, 32 * n)));
    }
    return decodePoints(N.msmBatch(ctx, points.handle, s, n, B, fb, opts), B);
  }

  // One MSM per segment (msmz_msm_segments): `segments` is an array of [firstPoint, firstScalar, n]; result k =
  // sum_{i < n} scalars[firstScalar + i] * points[firstPoint + i] over ONE resident scalar array and ONE resident point
  // array (plain or precomputed).  Checked here, before anything reaches the device.
  async function msmSegmentsCommon(scalars, points, segments, options, safe) {
    const opts = msmOpts(options || {}, "msmSegments", safe);
    if (!(points instanceof DeviceArray) || (points.kind !== "points" && points.kind !== "precomputed"))
      throw TypeError("msmSegments: `points` is a resident point array (plain or precomputed)");
    if (!isScalars(scalars))
      throw TypeError("msmSegments: `scalars` is a resident scalar array; host scalars are uploaded first");
    if (!Array.isArray(segments) || segments.length === 0 || segments.length >= 2 ** 32)
      throw Error("msmSegments: `segments` is a non-empty array of [firstPoint, firstScalar, n]");
    const table = Buffer.alloc(24 * segments.length);
    segments.forEach((seg, k) => {
      if (!Array.isArray(seg) || seg.length !== 3) throw TypeError(`msmSegments: segment ${k} is not [firstPoint, firstScalar, n]`);
      const [firstPoint, firstScalar, n] = seg;
      for (const v of seg) if (!Number.isInteger(v) || v < 0) throw Error(`msmSegments: segment ${k}: ${v}`);
      if (n < 1) throw Error(`msmSegments: segment ${k}: n = ${n}`);
      if (firstPoint + n > points.n) throw Error(`msmSegments: segment ${k}: points [${firstPoint}, +${n}) of a set of ${points.n}`);
      if (firstScalar + n > scalars.n) throw Error(`msmSegments: segment ${k}: scalars [${firstScalar}, +${n}) of a set of ${scalars.n}`);
      seg.forEach((v, j) => table.writeBigUInt64LE(BigInt(v), 24 * k + 8 * j));
    });
    return decodePoints(N.msmSegments(ctx, points.handle, scalars.handle, table, segments.length, fb, opts), segments.length);
  }

  const Parallel = {
    /** fixed-base precomputation of the first n resident points (include/msmz.h msmz_precompute_points): a DeviceArray
     * of kind "precomputed" that msm / msmUnsafe / msmBatch / msmBatchUnsafe take in place of the points (same results).
     * factor = windows sharing one bucket set (0 = all; 1 is refused); options.c / options.glv fix the window size and
     * the GLV choice (default: the engine's), options.scalarBits the scalar bit bound the copies are built for (fewer
     * windows, fewer copies; MSMs over the array take that bound).  The copies' parameters are in the array's `info`. */
    async precomputePoints(points, n, options, factor = 0) {
      options = options || {};
      if (!isPoints(points))
        throw TypeError("precomputePoints: `points` is a resident point array (pointsFromBytes / randomPointsFast)");
      if (!Number.isInteger(n) || n < 1 || n > points.n) throw Error(`precomputePoints: n = ${n} but the point set holds ${points.n}`);
      if (!Number.isInteger(factor) || factor < 0 || factor === 1 || factor >= 2 ** 32)
        throw Error(`precomputePoints: factor = ${factor} (0 = all windows, or 2, 3, ...)`);
      const opts = { c: options.c || 0, glv: options.glv !== undefined ? Number(options.glv) : -1,
                     scalarBits: scalarBitsArg(options, "precomputePoints") };
      const h = N.precomputePoints(ctx, points.handle, n, opts, factor);
      const arr = DeviceArray.make(curve, h, n, "precomputed");
      Object.defineProperty(arr, "info", { value: N.precomputedInfo(ctx, h) });
      return arr;
    },
    /** validation of a resident point set (include/msmz.h msmz_check_points): are points [first, first + n) on the curve
     * and, with subgroup (the default), in the subgroup of prime order?  isOnCurve / isInSubgroup of the reference's
     * curve API over a whole set, on the GPU.  -> {ok, offCurve, offSubgroup, firstBad (an index of the array, null if
     * ok), verdicts (with options.verdicts: one byte per point, bit 0 = not on the curve, bit 1 = on the curve but
     * outside the subgroup)} */
    async checkPoints(points, n, { subgroup = true, first = 0, verdicts = false } = {}) {
      if (!isPoints(points))
        throw TypeError("checkPoints: `points` is a resident point array (pointsFromBytes / randomPointsFast)");
      if (!Number.isInteger(first) || first < 0 || first >= points.n) throw Error(`checkPoints: first = ${first} but the point set holds ${points.n}`);
      n = n === undefined || n === null ? points.n - first : n;
      if (!Number.isInteger(n) || n < 1 || n > points.n - first) throw Error(`checkPoints: points [${first}, +${n}) of a set of ${points.n}`);
      const r = N.checkPoints(ctx, points.handle, first, n, subgroup ? 3 : 1, !!verdicts);
      return { ok: r.firstBad < 0, offCurve: r.offCurve, offSubgroup: r.offSubgroup, firstBad: r.firstBad < 0 ? null : r.firstBad,
               verdicts: r.verdicts };
    },
    /** per-point scalar multiplication (include/msmz.h msmz_points_mul): a new resident point array,
     * out[i] = [s_i] points[firstPoint + i] (+ addend[firstAddend + i]), i < n.  `scalars` is a resident scalar array
     * (s_i = scalars[firstScalar + i]) or a bigint below the group order: one scalar for every point.  `addend` may be
     * `points` itself (an IPA fold: mulPoints(u, G, n, {addend: G, firstPoint: n})).  The result is an ordinary point
     * array.  scalarBits = b: every scalar of the call is below 2^b and the chain walks b bits only (0 = no bound; a
     * scalar that breaks it fails the call).  subgroup: the caller vouches that every finite point of the range lies
     * in the prime-order subgroup (checkPoints says so); the Weierstrass curves then run the GLV chain, about half as
     * long, and for a point outside the subgroup that row of the result is unspecified. */
    async mulPoints(scalars, points, n, { addend = null, firstPoint = 0, firstScalar = 0, firstAddend = 0, scalarBits = 0,
                                          subgroup = false } = {}) {
      if (!isPoints(points))
        throw TypeError("mulPoints: `points` is a resident point array (pointsFromBytes / randomPointsFast)");
      if (addend !== null && !isPoints(addend))
        throw TypeError("mulPoints: `addend` is a resident point array or null");
      const broadcast = typeof scalars === "bigint";
      if (!broadcast && !isScalars(scalars))
        throw TypeError("mulPoints: `scalars` is a resident scalar array or a bigint (one scalar for every point)");
      if (broadcast && (scalars < 0n || scalars >= params.order)) throw Error(`mulPoints: the scalar ${scalars} is not in [0, group order)`);
      n = scanRanges("mulPoints", [["firstPoint", firstPoint, points], ["firstScalar", firstScalar, broadcast ? null : scalars],
                                   ["firstAddend", firstAddend, addend]], n, null, Infinity);   // (no bound on n here)
      if (typeof subgroup !== "boolean") throw TypeError(`mulPoints: subgroup = ${subgroup} (true: every point lies in the prime-order subgroup)`);
      const bits = scalarBitsArg({ scalarBits }, "mulPoints");
      if (bits && broadcast && scalars >> BigInt(bits)) throw Error(`mulPoints: the scalar ${scalars} is not below 2^${bits} (scalarBits)`);
      const h = N.mulPoints(ctx, points.handle, firstPoint, broadcast ? scalarBuf(scalars) : scalars.handle,
                            firstScalar, addend === null ? 0 : addend.handle, firstAddend, n, bits, subgroup ? 1 : 0);
      return DeviceArray.make(curve, h, n, "points");
    },
    /** fixed-base multiplication (include/msmz.h msmz_points_fixed_base): a new resident point array,
     * out[i] = [scalars[firstScalar + i]] B, i < n, for ONE base B -- an SRS [tau^i]G from scalarPowers(tau, n), Pedersen
     * vectors, points with known discrete logs.  `base`: null (the curve's generator), an affine point {x, y, isZero},
     * or a resident point array, of which B is point `baseIndex`.  B need not lie in the subgroup.  The result is what
     * mulPoints leaves for n copies of B, from a window table of multiples of B (kept for the next call on the same
     * base) instead of a chain per point.  scalarBits = b: every scalar of the range is below 2^b (0 = no bound; a
     * scalar that breaks it fails the call). */
    async fixedBaseMul(scalars, n, { base = null, baseIndex = 0, firstScalar = 0, scalarBits = 0 } = {}) {
      if (!isScalars(scalars)) throw TypeError("fixedBaseMul: `scalars` is a resident scalar array");
      let b = null;
      if (isPoints(base)) {
        if (!Number.isInteger(baseIndex) || baseIndex < 0 || baseIndex >= base.n)
          throw Error(`fixedBaseMul: baseIndex = ${baseIndex} of a point array of ${base.n}`);
        b = base.handle;
      } else if (base !== null) {
        if (typeof base !== "object" || base instanceof DeviceArray || typeof base.x !== "bigint" || typeof base.y !== "bigint")
          throw TypeError("fixedBaseMul: `base` is null (the generator), an affine point {x, y, isZero} or a resident point array");
        if (baseIndex !== 0) throw Error("fixedBaseMul: baseIndex without a resident point array");
        const zero = !!base.isZero;
        for (const v of [base.x, base.y])
          if (!zero && (v < 0n || v >= params.modulus)) throw Error("fixedBaseMul: a coordinate of the base is not in [0, field modulus)");
        b = zero ? Buffer.alloc(2 * fb) : Buffer.concat([bigintToBytes(base.x, fb), bigintToBytes(base.y, fb)]);
      } else if (baseIndex !== 0) {
        throw Error("fixedBaseMul: baseIndex without a resident point array");
      }
      n = scanRanges("fixedBaseMul", [["firstScalar", firstScalar, scalars]], n, null, Infinity);
      const bits = scalarBitsArg({ scalarBits }, "fixedBaseMul");
      const h = N.fixedBaseMul(ctx, scalars.handle, firstScalar, n, b, isPoints(base) ? baseIndex : 0, bits);
      return DeviceArray.make(curve, h, n, "points");
    },
    /** arithmetic mod the group order over resident scalar arrays (include/msmz.h msmz_scalars_combine):
     * out[firstOut + i] = a_i x[firstX + i] (+ b_i y[firstY + i]), i < n.  `a` and `b` are bigints below the group order
     * (one coefficient for every entry) or resident scalar arrays (a_i = a[firstA + i]).  Without `out` the result is a
     * new scalar array; with it, entries [firstOut, firstOut + n) of `out` are overwritten, and `out` may be an input
     * when the range is exactly that input's or apart from it (an IPA fold in place:
     * combineScalars(1n, v, uinv, v, n, {firstY: n, out: v})).  Returns the array written. */
    async combineScalars(a, x, b = null, y = null, n, { firstX = 0, firstY = 0, out = null, firstOut = 0, firstA = 0, firstB = 0 } = {}) {
      if (!isScalars(x)) throw TypeError("combineScalars: `x` is a resident scalar array");
      if ((b === null) !== (y === null)) throw TypeError("combineScalars: `b` and `y` come together");
      if (y !== null && !isScalars(y)) throw TypeError("combineScalars: `y` is a resident scalar array or null");
      if (out !== null && !isScalars(out)) throw TypeError("combineScalars: `out` is a resident scalar array or null");
      const ranges = [["firstX", firstX, x], ["firstY", firstY, y]];
      const coeff = (name, c, first, used) => {
        if (!used) { ranges.push([name, first, null]); return null; }
        if (typeof c === "bigint") {
          if (c < 0n || c >= params.order) throw Error(`combineScalars: the coefficient ${c} is not in [0, group order)`);
          ranges.push([name, first, null]);
          return c === 1n ? null : scalarBuf(c);
        }
        if (!isScalars(c)) throw TypeError("combineScalars: a coefficient is a bigint (one for every entry) or a resident scalar array");
        ranges.push([name, first, c]);
        return c.handle;
      };
      const ca = coeff("firstA", a, firstA, true), cb = coeff("firstB", b, firstB, y !== null);
      ranges.push(["firstOut", firstOut, out]);
      n = scanRanges("combineScalars", ranges, n, out);
      const h = N.scalarsCombine(ctx, x.handle, firstX, ca, firstA, y === null ? 0 : y.handle, firstY, cb, firstB, n, firstOut,
                                 out === null ? 0 : out.handle);
      return out === null ? DeviceArray.make(curve, h, n, "scalars") : out;
    },
    /** sum_i x[firstX + i] y[firstY + i] mod the group order (y null: sum_i x[firstX + i]) as a bigint
     * (msmz_scalars_dot); x and y may be one array and may overlap */
    async innerProduct(x, y = null, n, { firstX = 0, firstY = 0 } = {}) {
      if (!isScalars(x) || (y !== null && !isScalars(y))) throw TypeError("innerProduct: `x` and `y` are resident scalar arrays (y may be null)");
      n = scanRanges("innerProduct", [["firstX", firstX, x], ["firstY", firstY, y]], n);
      const r = N.scalarsDot(ctx, x.handle, firstX, y === null ? 0 : y.handle, firstY, n);
      return bytesToBigint(r, 0, 32);
    },
    /** every inner product of a family of row vectors with a family of column vectors in one call
     * (msmz_scalars_dot_many): result[r][c] = sum_i rows[r][i] cols[c][i] mod the group order, i < n, each what
     * innerProduct gives for that pair.  rows (1 to 128) and cols (1 to 8): resident scalar arrays or [array, first]
     * pairs; they may share arrays, overlap and be one range.  n null: what the shortest vector leaves.  Without `out`:
     * an array of rows.length arrays of bigints.  With `out`, a resident scalar array, entries [firstOut, firstOut +
     * rows.length cols.length) of it receive the values row-major (the range meets no input range) and `out` comes
     * back.  Many multilinear tables at one point: eqTable(point), then innerProducts(tables, [eq]). */
    async innerProducts(rows, cols, n = null, options = {}) {
      const t = dotManyArgs(rows, cols, n, options);
      for (const [arr] of [...t.rows, ...t.cols]) if (!isScalars(arr)) throw TypeError("innerProducts: a vector is a resident scalar array");
      const pack = (pairs) => {
        const b = Buffer.alloc(16 * pairs.length);
        pairs.forEach(([arr, first], j) => {
          b.writeBigUInt64LE(BigInt(arr.handle), 16 * j);
          b.writeBigUInt64LE(BigInt(first), 16 * j + 8);
        });
        return b;
      };
      const out = options.out === undefined ? null : options.out, nr = t.rows.length, nc = t.cols.length;
      if (out !== null) {
        if (!isScalars(out)) throw TypeError("innerProducts: `out` is a resident scalar array");
        N.scalarsDotMany(ctx, pack(t.rows), nr, pack(t.cols), nc, t.n, 1, out.handle, t.firstOut);
        return out;
      }
      const r = N.scalarsDotMany(ctx, pack(t.rows), nr, pack(t.cols), nc, t.n, 0, 0, 0);
      return Array.from({ length: nr }, (_, j) => Array.from({ length: nc }, (_, c) => bytesToBigint(r, 32 * (j * nc + c), 32)));
    },
    /** result[r][c] = p_r(z_c) for polynomials in coefficient form: polys[r] a resident scalar array or [array, first]
     * pair whose entry i is the coefficient of X^i, i < n; points: 1 to 8 bigints below the group order.  One power
     * vector per point (scalarPowers), ONE innerProducts call, and the vectors are freed again.  In evaluation form the
     * same call serves: pass the barycentric weight vectors of the points as `cols` of innerProducts. */
    async evaluatePolynomials(polys, points, n = null) {
      const t = dotManyArgs(polys, Array.isArray(polys) ? polys.slice(0, 1) : polys, n, {}, "evaluatePolynomials");
      if (!Array.isArray(points) || !points.every((z) => typeof z === "bigint")) throw TypeError("evaluatePolynomials: `points` is an array of bigints");
      if (points.length < 1 || points.length > DOT_MANY_MAX_COLS) throw Error(`evaluatePolynomials: ${points.length} points (1 to ${DOT_MANY_MAX_COLS})`);
      for (const z of points) if (z < 0n || z >= params.order) throw Error(`evaluatePolynomials: the point ${z} is not in [0, group order)`);
      const powers = [];
      try {
        for (const z of points) powers.push(await Parallel.scalarPowers(z, t.n));
        return await Parallel.innerProducts(t.rows, powers, t.n);
      } finally {
        for (const a of powers) a.free();
      }
    },
    /** a new resident scalar array: entry i = base ratio^i mod the group order (msmz_scalars_powers; 0^0 = 1) */
    async scalarPowers(ratio, n, base = 1n) {
      for (const [name, v] of [["ratio", ratio], ["base", base]]) {
        if (typeof v !== "bigint") throw TypeError(`scalarPowers: \`${name}\` is a bigint`);
        if (v < 0n || v >= params.order) throw Error(`scalarPowers: ${name} = ${v} is not in [0, group order)`);
      }
      if (!Number.isInteger(n) || n < 1 || n >= 2 ** 32) throw Error(`scalarPowers: n = ${n}`);
      const h = N.scalarsPowers(ctx, scalarBuf(base), scalarBuf(ratio), n);
      return DeviceArray.make(curve, h, n, "scalars");
    },
    /** the first-order linear recurrence y_i = a_i y_(i-1) + b_i mod the group order, i < n, from y_(-1) = init
     * (include/msmz.h msmz_scalars_recurrence; reverse: y_i = a_i y_(i+1) + b_i from y_n = init).  `a`: a resident scalar
     * array (a_i = a[firstA + i]), a bigint (one multiplier for every entry) or null (1); `b`: a resident scalar array or
     * null (no addend); not both null.  init null: 0n with an addend, 1n without.  out[firstOut + i] = y_i, or with
     * `exclusive` the value the step at i started from.  Without `out` the result is a new array; `out` may be `a` or `b`
     * when the range is exactly theirs or apart from it.  Returns [the array written, the final y]. */
    async scalarRecurrence(a, b, n, { init = null, reverse = false, exclusive = false, firstA = 0, firstB = 0, out = null, firstOut = 0 } = {}) {
      const broadcast = typeof a === "bigint";
      if (a !== null && !broadcast && !isScalars(a)) throw TypeError("scalarRecurrence: `a` is a resident scalar array, a bigint or null");
      if (b !== null && !isScalars(b)) throw TypeError("scalarRecurrence: `b` is a resident scalar array or null");
      if (a === null && b === null) throw TypeError("scalarRecurrence: neither a multiplier nor an addend");
      if (out !== null && !isScalars(out)) throw TypeError("scalarRecurrence: `out` is a resident scalar array or null");
      if (init !== null && typeof init !== "bigint") throw TypeError("scalarRecurrence: `init` is a bigint or null");
      for (const [name, v] of [["a", broadcast ? a : null], ["init", init]])
        if (v !== null && (v < 0n || v >= params.order)) throw Error(`scalarRecurrence: ${name} = ${v} is not in [0, group order)`);
      n = scanRanges("scalarRecurrence", [["firstA", firstA, isScalars(a) ? a : null], ["firstB", firstB, b], ["firstOut", firstOut, out]], n, out);
      const r = N.scalarsRecurrence(ctx, broadcast ? scalarBuf(a) : a === null ? null : a.handle, firstA,
                                    b === null ? 0 : b.handle, firstB, init === null ? null : scalarBuf(init),
                                    (reverse ? 1 : 0) | (exclusive ? 2 : 0), n, firstOut, out === null ? 0 : out.handle);
      return [out === null ? DeviceArray.make(curve, r.handle, n, "scalars") : out, bytesToBigint(r.last, 0, 32)];
    },
    /** running products of x[first + i]: [array, the full product]; exclusive: entry 0 is 1 (a grand product column) */
    prefixProducts(x, n, { exclusive = false, init = null, reverse = false, first = 0, out = null, firstOut = 0 } = {}) {
      return this.scalarRecurrence(x, null, n, { init, reverse, exclusive, firstA: first, out, firstOut });
    },
    /** running sums of x[first + i]: [array, the full sum] */
    prefixSums(x, n, { exclusive = false, init = null, reverse = false, first = 0, out = null, firstOut = 0 } = {}) {
      return this.scalarRecurrence(null, x, n, { init, reverse, exclusive, firstB: first, out, firstOut });
    },
    /** (p(X) - p(z)) / (X - z) for the coefficients p[first + i], i < n, lowest degree first: [quotient, p(z)].  The
     * quotient has n entries, the top one 0: an MSM takes it against the same n points as p (a KZG opening proof). */
    async divideByLinear(p, z, n, { first = 0 } = {}) {
      if (typeof z !== "bigint") throw TypeError("divideByLinear: `z` is a bigint");
      if (!isScalars(p)) throw TypeError("divideByLinear: `p` is a resident scalar array");
      return this.scalarRecurrence(z, p, n, { init: 0n, reverse: true, exclusive: true, firstB: first });
    },
    /** out[firstOut + i] = x[first + i]^-1 mod the group order, 0 -> 0 (msmz_scalars_inverse): [the array written, the
     * number of zeros].  `out` may be `x` over exactly the same range (in place) or apart from it. */
    async invertScalars(x, n, { first = 0, out = null, firstOut = 0 } = {}) {
      if (!isScalars(x)) throw TypeError("invertScalars: `x` is a resident scalar array");
      if (out !== null && !isScalars(out)) throw TypeError("invertScalars: `out` is a resident scalar array or null");
      n = scanRanges("invertScalars", [["first", first, x], ["firstOut", firstOut, out]], n, out);
      const r = N.scalarsInverse(ctx, x.handle, first, n, firstOut, out === null ? 0 : out.handle);
      return [out === null ? DeviceArray.make(curve, r.handle, n, "scalars") : out, r.zeros];
    },
    /** `count` number-theoretic transforms of length n = 2^logN mod the group order, natural order in and out
     * (include/msmz.h msmz_scalars_ntt).  Input vector k is x[first + k nIn .. first + (k + 1) nIn) continued with zeros
     * (nIn null: n), output vector k is out[firstOut + k n .. firstOut + (k + 1) n).  Forward: out_k = sum_i x_i (g w^k)^i;
     * inverse: x_i = g^-i n^-1 sum_k X_k w^(-i k).  `shift` is the coset shift g (a bigint, not 0n; null: 1), `root` a
     * primitive n-th root of unity (null: rootOfUnity(logN)).  Without `out` the result is a new array of count n entries;
     * `out` may be `x` over exactly the source range (in place, nIn = n) or apart from it.  Returns the array written. */
    async ntt(x, logN, options = {}) {
      if (!isScalars(x)) throw TypeError("ntt: `x` is a resident scalar array");
      if (options.out !== undefined && options.out !== null && !isScalars(options.out)) throw TypeError("ntt: `out` is a resident scalar array or null");
      const t = nttArgs(x, logN, options, params.order);
      const out = options.out === undefined ? null : options.out;
      const h = N.scalarsNtt(ctx, x.handle, t.first, t.logN, t.flags, t.nIn, t.count, t.root === null ? null : scalarBuf(t.root),
                             t.shift === null ? null : scalarBuf(t.shift), t.firstOut, out === null ? 0 : out.handle);
      return out === null ? DeviceArray.make(curve, h, t.count * 2 ** t.logN, "scalars") : out;
    },
    /** the default primitive 2^logN-th root of unity of the scalar field as a bigint (msmz_scalars_root_of_unity) */
    rootOfUnity(logN) {
      if (!Number.isInteger(logN) || logN < 0 || logN >= 2 ** 32) throw Error(`rootOfUnity: logN = ${logN}`);
      return bytesToBigint(N.scalarsRootOfUnity(params.curveId, logN), 0, 32);
    },
    /** a new resident scalar array of 2^point.length entries: entry i = scale eq(point, i) mod the group order, eq(r, i) =
     * prod_j (b_j r_j + (1 - b_j)(1 - r_j)) over the bits b_j of i, variable 0 the lowest bit (msmz_scalars_eq_table) */
    async eqTable(point, scale = 1n) {
      const t = eqTableArgs(point, scale, params.order);
      const h = N.scalarsEqTable(ctx, Buffer.concat(point.map(scalarBuf)), t.nVars, t.scale === null ? null : scalarBuf(t.scale));
      return DeviceArray.make(curve, h, 2 ** t.nVars, "scalars");
    },
    /** f(point) = sum_i f[first + i] eq(point, i) over 2^point.length entries as a bigint; the eq table is not made
     * (msmz_scalars_mle_eval) */
    async evaluateMle(f, point, options = {}) {
      if (!isScalars(f)) throw TypeError("evaluateMle: `f` is a resident scalar array");
      const t = mleEvalArgs(f, point, options, params.order);
      return bytesToBigint(N.scalarsMleEval(ctx, f.handle, t.first, Buffer.concat(point.map(scalarBuf)), t.nVars), 0, 32);
    },
    /** binds one variable of `count` tables of 2^nVars entries (table k at f[first + k 2^nVars]) to the bigint r
     * (msmz_scalars_mle_bind): out_i = f_i + r (f_(i+h) - f_i), h = 2^(nVars-1), or with `low` out_i = f_(2i) +
     * r (f_(2i+1) - f_(2i)).  Without `out` the result is a new array of count h entries; `out` may be `f` only with
     * count 1, the high variable and firstOut == first (the low half is overwritten), or over a range apart from the
     * source.  Returns the array written. */
    async bindMle(f, r, options = {}) {
      if (!isScalars(f)) throw TypeError("bindMle: `f` is a resident scalar array");
      if (options.out !== undefined && options.out !== null && !isScalars(options.out)) throw TypeError("bindMle: `out` is a resident scalar array or null");
      const t = mleBindArgs(f, r, options, params.order);
      const out = options.out === undefined ? null : options.out;
      const h = N.scalarsMleBind(ctx, f.handle, t.first, t.nVars, t.count, t.flags, scalarBuf(r), t.firstOut, out === null ? 0 : out.handle);
      return out === null ? DeviceArray.make(curve, h, t.n, "scalars") : out;
    },
    /** the round polynomial of a sumcheck over sum_i sum_T c_T prod_(j in T) tables[j][i] (msmz_scalars_sumcheck_round):
     * an array of d + 1 bigints g(0) .. g(d).  `tables`: 1 to 6 resident scalar arrays or [array, first] pairs; `terms`:
     * 1 to 8 pairs [c, mask], c a bigint or null (1), bit j of mask making table j a factor, at most 4 factors; d = the
     * most factors of a term.  The round sums out the high variable, with `low` variable 0; bindMle with the same `low`
     * goes on to the next round. */
    async sumcheckRound(tables, terms, options = {}) {
      const t = sumcheckRoundArgs(tables, terms, options, params.order);
      for (const [arr] of t.tables) if (!isScalars(arr)) throw TypeError("sumcheckRound: a table is a resident scalar array");
      const tb = Buffer.alloc(16 * t.tables.length), masks = Buffer.alloc(4 * t.terms.length), unit = Buffer.alloc(t.terms.length);
      t.tables.forEach(([arr, first], j) => {
        tb.writeBigUInt64LE(BigInt(arr.handle), 16 * j);
        tb.writeBigUInt64LE(BigInt(first), 16 * j + 8);
      });
      const coeffs = Buffer.concat(t.terms.map(([c, mask], k) => {
        masks.writeUInt32LE(mask, 4 * k);
        unit[k] = c === null ? 1 : 0;
        return scalarBuf(c === null ? 1n : c);
      }));
      const r = N.scalarsSumcheckRound(ctx, tb, t.tables.length, t.nVars, masks, coeffs, unit, t.terms.length, t.flags);
      return Array.from({ length: r.length / 32 }, (_, k) => bytesToBigint(r, 32 * k, 32));
    },
    /** one step of a sumcheck prover in one call (msmz_scalars_sumcheck_step): binds every table of 2^nVars entries to the
     * bigint r, as bindMle with the same `low` does, and returns {degree, values}, the polynomial sumcheckRound gives over
     * the bound tables.  options: {nVars, out, low}; `out`: one resident scalar array or [array, first] pair per table,
     * each apart from every other destination and every other table, and apart from its own table or exactly its low
     * half (high order only); without `out` every table is bound in place (high order only).  nVars 1 is the last step:
     * {degree: 0, values: [the final claim]}. */
    async sumcheckStep(tables, terms, r, options = {}) {
      const t = sumcheckStepArgs(tables, terms, r, options, params.order);
      for (const [arr] of [...t.tables, ...(t.out || [])]) if (!isScalars(arr)) throw TypeError("sumcheckStep: a table is a resident scalar array");
      const pack = (pairs) => {
        const b = Buffer.alloc(16 * pairs.length);
        pairs.forEach(([arr, first], j) => {
          b.writeBigUInt64LE(BigInt(arr.handle), 16 * j);
          b.writeBigUInt64LE(BigInt(first), 16 * j + 8);
        });
        return b;
      };
      const masks = Buffer.alloc(4 * t.terms.length), unit = Buffer.alloc(t.terms.length);
      const coeffs = Buffer.concat(t.terms.map(([c, mask], k) => {
        masks.writeUInt32LE(mask, 4 * k);
        unit[k] = c === null ? 1 : 0;
        return scalarBuf(c === null ? 1n : c);
      }));
      const res = N.scalarsSumcheckStep(ctx, pack(t.tables), t.out === null ? null : pack(t.out), t.tables.length, t.nVars, masks,
        coeffs, unit, t.terms.length, t.flags, scalarBuf(r));
      const values = Array.from({ length: res.length / 32 }, (_, k) => bytesToBigint(res, 32 * k, 32));
      return { degree: values.length - 1, values };
    },
    /** the prover's side of a whole sumcheck: one sumcheckRound, then one sumcheckStep per variable with r =
     * await challenge(values of the round before), a bigint below the group order -- the transcript is the caller's.
     * Returns {polys, challenges, claim}.  A host loop and nothing else; the tables are consumed: in the high order they
     * are bound in place, with `low` the steps go back and forth between each table and one scratch array per table,
     * allocated here and freed before returning.  The tables lie apart from each other. */
    async sumcheckProve(tables, terms, nVars, challenge, { low = false } = {}) {
      const t = sumcheckRoundArgs(tables, terms, { nVars, low }, params.order, "sumcheckProve");
      if (typeof challenge !== "function") throw TypeError("sumcheckProve: `challenge` is a function of the round's values returning a bigint");
      let cur = t.tables;
      const polys = [await Parallel.sumcheckRound(cur, terms, { nVars: t.nVars, low })], challenges = [];
      let claim = null, spare = [];
      try {
        if (low) spare = cur.map(() => DeviceArray.make(curve, N.allocScalars(ctx, 2 ** (t.nVars - 1)), 2 ** (t.nVars - 1), "scalars"));
        let other = spare.map((a) => [a, 0]);
        for (let v = t.nVars; v >= 1; v--) {
          const r = await challenge([...polys[polys.length - 1]]);
          const { values } = await Parallel.sumcheckStep(cur, terms, r, { nVars: v, out: low ? other : null, low });
          challenges.push(r);
          if (v > 1) polys.push(values);
          else claim = values[0];
          if (low) [cur, other] = [other, cur];
        }
      } finally {
        for (const a of spare) a.free();
      }
      return { polys, challenges, claim };
    },
    /** a resident sparse matrix of shape [nRows, nCols] from triples (rows[k], cols[k], values[k]) in any order, triples
     * with the same (row, col) adding up (msmz_matrix_create).  values: a resident scalar array (value k =
     * values[firstValue + k]), an array of bigints below the group order (uploaded first, freed afterwards) or null:
     * every value is 1.  options: {shape, orientations: "rows" (for matVec) | "cols" (for transpose) | "both", firstValue} */
    async sparseMatrix(rows, cols, values = null, options = {}) {
      let vals = values, mine = false;
      if (Array.isArray(values) && !(values instanceof DeviceArray)) {
        values.forEach((v, k) => {
          if (typeof v !== "bigint") throw TypeError("sparseMatrix: a value is a bigint");
          if (v < 0n || v >= params.order) throw Error(`sparseMatrix: values[${k}] = ${v} is not in [0, group order)`);
        });
        if (values.length !== rows.length) throw Error(`sparseMatrix: ${rows.length} rows but ${values.length} values`);
        if ((options.firstValue || 0) !== 0) throw Error(`sparseMatrix: firstValue = ${options.firstValue} without the array it indexes`);
        sparseMatrixArgs(rows, cols, null, options);   // (every host check before the upload)
        vals = await Parallel.scalarsFromBytes(Buffer.concat(values.map(scalarBuf)));
        mine = true;
      }
      try {
        const t = sparseMatrixArgs(rows, cols, vals, options);
        if (vals !== null && !isScalars(vals)) throw TypeError("sparseMatrix: `values` is a resident scalar array, an array of bigints or null");
        const h = N.matrixCreate(ctx, t.rows, t.cols, t.nnz, vals === null ? 0 : vals.handle, t.firstValue, t.shape[0], t.shape[1], t.flags);
        return new SparseMatrix(curve, h, t.shape, t.nnz, options.orientations === undefined ? "rows" : options.orientations);
      } finally {
        if (mine) vals.free();
      }
    },
    /** out[firstOut + i] = sum over the non-zeros (i, j, v) of v x[firstX + j] mod the group order; with `transpose` over
     * (j, i, v) (msmz_matrix_mul).  Without `out` a new array; `out` may be `x` only over a range that does not meet the
     * x range.  options: {firstX, transpose, out, firstOut}.  Returns the array written. */
    async matVec(matrix, x, options = {}) {
      const t = matVecArgs(matrix, x, options);
      if (!(matrix instanceof SparseMatrix) || !isScalars(x)) throw TypeError("matVec: a sparse matrix and a resident scalar array");
      const out = options.out === undefined ? null : options.out;
      if (out !== null && !isScalars(out)) throw TypeError("matVec: `out` is a resident scalar array or null");
      const h = N.matrixMul(ctx, matrix.handle, x.handle, options.firstX || 0, t.flags, options.firstOut || 0, out === null ? 0 : out.handle);
      return out === null ? DeviceArray.make(curve, h, t.n, "scalars") : out;
    },
    /** [m, info] for the column f = column[firstColumn, +n) and the table t = table[firstTable, +tableN): m a resident
     * scalar array of tableN entries, m[j] = #{i : f[i] = t[j]} if j is the lowest index among the table entries that hold
     * t[j] and 0 for every later duplicate -- the vector a logUp argument commits to (msmz_scalars_lookup).  info =
     * {missing, firstMissing (null if none), distinct} and, with positions: true, positions: a Uint32Array, the index of
     * the first table entry equal to f[i] or 0xffffffff.  A column entry that is in no table is not an error.  `out` may
     * meet neither the table range nor the column range of the same array.
     * options: {firstColumn, n, firstTable, tableN, out, firstOut, positions} */
    async lookupMultiplicities(column, table, options = {}) {
      const t = lookupArgs(column, table, options);
      if (!isScalars(column) || !isScalars(table)) throw TypeError("lookupMultiplicities: resident scalar arrays");
      const out = options.out === undefined ? null : options.out;
      if (out !== null && !isScalars(out)) throw TypeError("lookupMultiplicities: `out` is a resident scalar array or null");
      const r = N.scalarsLookup(ctx, table.handle, options.firstTable || 0, t.tableN, column.handle, options.firstColumn || 0, t.n,
                                options.firstOut || 0, out === null ? 0 : out.handle, options.positions === true);
      const info = { missing: r.missing, firstMissing: r.firstMissing < 0 ? null : r.firstMissing, distinct: r.distinct };
      if (r.positions !== null) {
        info.positions = new Uint32Array(t.n);
        for (let i = 0; i < t.n; i++) info.positions[i] = r.positions.readUInt32LE(4 * i);
      }
      return [out === null ? DeviceArray.make(curve, r.handle, t.tableN, "scalars") : out, info];
    },
    /** out[firstOut + i] = sum_T c_T prod_(f in T) column_f[(i + rot_f) mod n] mod the group order, i < n: the constraint
     * expression of a PLONK-ish prover entry by entry, in one launch (msmz_scalars_expr).  columns: 1 to 16 resident
     * scalar arrays or [array, first] pairs; terms: 1 to 32 pairs [c, factors], c a bigint below the group order or null
     * (1), factors an array of at most 8 column indices or [column, rot] pairs ([] makes the term the constant c; a
     * factor may repeat).  A rotation is cyclic inside the column's n entries and any int32; over an extended coset of
     * size 4 n pass 4 rot.  At most 32 distinct (column, rot mod n) pairs in all.  Without `out` a new array; `out` may
     * be a column read at rotation 0 only, over exactly its range (out = y out + gate is the term [y, [out]] next to the
     * gate's, in place), or apart from every column the terms read.  options: {n, out, firstOut}.  Returns the array written. */
    async evaluateExpression(columns, terms, options = {}) {
      const t = exprArgs(columns, terms, options, params.order);
      for (const [arr] of t.columns) if (!isScalars(arr)) throw TypeError("evaluateExpression: a column is a resident scalar array");
      const out = options.out === undefined ? null : options.out;
      if (out !== null && !isScalars(out)) throw TypeError("evaluateExpression: `out` is a resident scalar array or null");
      const cb = Buffer.alloc(16 * t.columns.length), counts = Buffer.alloc(t.terms.length), unit = Buffer.alloc(t.terms.length);
      t.columns.forEach(([arr, first], j) => {
        cb.writeBigUInt64LE(BigInt(arr.handle), 16 * j);
        cb.writeBigUInt64LE(BigInt(first), 16 * j + 8);
      });
      const fb = Buffer.alloc(8 * Math.max(1, t.terms.reduce((s, [, fs]) => s + fs.length, 0)));
      let at = 0;
      const coeffs = Buffer.concat(t.terms.map(([c, fs], k) => {
        counts[k] = fs.length;
        unit[k] = c === null ? 1 : 0;
        for (const [col, rot] of fs) {
          fb.writeUInt32LE(col, 8 * at);
          fb.writeInt32LE(rot, 8 * at + 4);
          at++;
        }
        return scalarBuf(c === null ? 1n : c);
      }));
      const h = N.scalarsExpr(ctx, cb, t.columns.length, fb, counts, coeffs, unit, t.terms.length, t.n, options.firstOut || 0,
                              out === null ? 0 : out.handle);
      return out === null ? DeviceArray.make(curve, h, t.n, "scalars") : out;
    },
    /** batched MSM: B scalar vectors against one point set (include/msmz.h msmz_msm_batch); safe additions */
    msmBatch: (scalarsList, points, n, options) => msmBatchCommon(scalarsList, points, n, options, 1),
    msmBatchUnsafe: (scalarsList, points, n, options) => msmBatchCommon(scalarsList, points, n, options, 0),
    /** segmented MSM: every problem its own range [firstPoint, firstScalar, n] of one point set and one scalar set
     * (include/msmz.h msmz_msm_segments), e.g. the L and R of an IPA round: [[n, 0, n], [0, n, n]]; safe additions */
    msmSegments: (scalars, points, segments, options) => msmSegmentsCommon(scalars, points, segments, options, 1),
    msmSegmentsUnsafe: (scalars, points, segments, options) => msmSegmentsCommon(scalars, points, segments, options, 0),
    /** curve-random.ts:14-92, seeded: point i = splitmix64(seed, i) * G */
    async randomPointsFast(n, { seed = 0x6d736d7an } = {}) {
      return DeviceArray.make(curve, N.randomPoints(ctx, n, BigInt(seed)), n, "points");
    },
    /** curve-random.ts:151-194, seeded */
    async randomScalars(n, { seed = 0x6d736d7an } = {}) {
      return DeviceArray.make(curve, N.randomScalars(ctx, n, BigInt(seed)), n, "scalars");
    },
    /** parallel.ts:89-95 */
    async getPointer(size) { return space.alloc(size, "field"); },
    async getScalarPointer(size) { return space.alloc(size, "scalar"); },
    /** parallel.ts:97-112: x||y little-endian canonical.  Two forms: (bytes, n?, isInf?) -> DeviceArray, and the
     * reference's (pointPtr, pointInputPtr, n): the bytes were put behind pointInputPtr with Field.memoryBytes.set,
     * the converted (Montgomery, GPU-resident) points end up behind pointPtr. */
    async pointsFromBytes(bytes, n, isInf) {
      if (typeof bytes === "number")   // (pointPtr, pointInputPtr, n)
        return fromPointer("pointsFromBytes", bytes, n, isInf, 2 * fb, (b) => N.uploadPoints(ctx, b, null, isInf), "points");
      // (bytes, n?, {montgomery, compressed, sign, isInf}): coordinates as 64-bit-limb Montgomery residues
      // v * 2^(8 feBytes) mod p; or compressed records of feBytes bytes, one coordinate (x; y on the twisted Edwards
      // curve) with the sign of the other in bit 7 of the last byte -- sign "largest": the canonical value is above
      // (p - 1) / 2, "parity": it is odd.  The GPU recovers the other coordinate; a record that is no point throws with
      // code "7".
      let montgomery = false, compressed = false, sign = "largest";
      if (isInf && typeof isInf === "object" && !ArrayBuffer.isView(isInf) && !Array.isArray(isInf)) {
        montgomery = !!isInf.montgomery;
        ({ compressed, sign } = compressedArgs("pointsFromBytes", isInf.compressed, isInf.sign, montgomery));
        isInf = isInf.isInf;
      }
      if (compressed) {
        n = n === undefined ? Math.floor(bytes.length / fb) : n;
        if (!(n > 0) || bytes.length < fb * n || (isInf && isInf.length < n)) throw Error(`pointsFromBytes: ${bytes.length} bytes for ${n} compressed points`);
        return DeviceArray.make(curve, N.importPointsCompressed(ctx, Buffer.from(bytes), isInf ? Buffer.from(isInf) : null, n, sign === "parity"), n, "points");
      }
      n = n === undefined ? Math.floor(bytes.length / (2 * fb)) : n;
      if (!(n > 0) || bytes.length < 2 * fb * n || (isInf && isInf.length < n)) throw Error(`pointsFromBytes: ${bytes.length} bytes for ${n} points`);
      if (montgomery) return DeviceArray.make(curve, N.importPoints(ctx, Buffer.from(bytes), isInf ? Buffer.from(isInf) : null, n, true), n, "points");
      return DeviceArray.make(curve, N.uploadPoints(ctx, Buffer.from(bytes), isInf ? Buffer.from(isInf) : null, n), n, "points");
    },
    /** points [first, first + count) of a resident point array as compressed records (msmz_download_points_compressed):
     * {records: Buffer of count * feBytes, isInf: Buffer of count}; infinity is an all-zero record with flag 1 */
    async pointsToCompressedBytes(points, { first = 0, count, sign } = {}) {
      if (!(points instanceof DeviceArray) || points.kind !== "points")
        throw TypeError("pointsToCompressedBytes: `points` is a resident point array (pointsFromBytes / randomPointsFast)");
      ({ sign } = compressedArgs("pointsToCompressedBytes", true, sign, false));
      count = count === undefined ? points.n - first : count;
      if (!Number.isInteger(first) || !Number.isInteger(count) || first < 0 || count <= 0 || first + count > points.n)
        throw Error(`pointsToCompressedBytes: points [${first}, +${count}) of an array of ${points.n}`);
      return N.downloadPointsCompressed(ctx, points.handle, first, count, fb, sign === "parity");
    },
    /** parallel.ts:114-133: 32 bytes little-endian per scalar */
    async scalarsFromBytes(bytes, n, count) {
      if (typeof bytes === "number")   // (scalarPtr, scalarInputPtr, n): parallel.ts:114-133
        return fromPointer("scalarsFromBytes", bytes, n, count, 32, (b) => N.uploadScalars(ctx, b, count), "scalars");
      // (bytes, n?, {width, montgomery}): `width` bytes per scalar on the wire (4..32, a multiple of 4, zero-extended on
      // the GPU); montgomery: 32-byte records v * 2^256 mod q.  Without them: the plain upload, as before.
      if (count && typeof count === "object") {
        const width = count.width === undefined ? 32 : count.width, montgomery = !!count.montgomery;
        if (!Number.isInteger(width) || width < 4 || width > 32 || width % 4) throw Error(`scalarsFromBytes: width = ${width} (4..32 bytes, a multiple of 4)`);
        if (montgomery && width !== 32) throw Error(`scalarsFromBytes: Montgomery scalars are 32-byte records, not ${width}`);
        if (width !== 32 || montgomery) {
          n = n === undefined ? Math.floor(bytes.length / width) : n;
          if (!(n > 0) || bytes.length < width * n) throw Error(`scalarsFromBytes: ${bytes.length} bytes for ${n} scalars of ${width} bytes`);
          return DeviceArray.make(curve, N.importScalars(ctx, Buffer.from(bytes), n, width, montgomery), n, "scalars");
        }
      }
      n = n === undefined ? Math.floor(bytes.length / 32) : n;
      if (!(n > 0) || bytes.length < 32 * n) throw Error(`scalarsFromBytes: ${bytes.length} bytes for ${n} scalars`);
      return DeviceArray.make(curve, N.uploadScalars(ctx, Buffer.from(bytes), n), n, "scalars");
    },
    /** entries [first, first + n) of a resident scalar array as n * width little-endian bytes (msmz_export_scalars, the
     * host route): only `width` bytes per scalar cross PCIe, and a scalar that does not fit them throws with code "6";
     * montgomery: 32-byte records v * 2^256 mod q in 64-bit limbs.  The defaults return what Scalar.toBigints reads. */
    async scalarsToBytes(scalars, { first = 0, n, width = 32, montgomery = false } = {}) {
      if (!(scalars instanceof DeviceArray) || scalars.kind !== "scalars")
        throw TypeError("scalarsToBytes: `scalars` is a resident scalar array");
      n = scanRanges("scalarsToBytes", [["first", first, scalars]], n);
      if (typeof montgomery !== "boolean") throw TypeError("scalarsToBytes: montgomery is true or false");
      if (!Number.isInteger(width) || width < 4 || width > 32 || width % 4) throw Error(`scalarsToBytes: width = ${width} (4..32 bytes, a multiple of 4)`);
      if (montgomery && width !== 32) throw Error(`scalarsToBytes: Montgomery scalars are 32-byte records, not ${width}`);
      return N.exportScalars(ctx, scalars.handle, first, n, width, montgomery);
    },
    /** points [first, first + n) of a resident point array (msmz_export_points, the host route): {records: Buffer of
     * n * 2 * feBytes (x || y; montgomery: coordinates v * 2^(8 feBytes) mod p in 64-bit limbs), isInf: Buffer of n};
     * infinity is an all-zero record with flag 1.  pointsFromBytes(records, n, {montgomery, isInf}) reads them back. */
    async pointsToBytes(points, { first = 0, n, montgomery = false } = {}) {
      if (!(points instanceof DeviceArray) || points.kind !== "points")
        throw TypeError("pointsToBytes: `points` is a resident point array (pointsFromBytes / randomPointsFast)");
      n = scanRanges("pointsToBytes", [["first", first, points]], n, null, 2 ** 31);
      if (typeof montgomery !== "boolean") throw TypeError("pointsToBytes: montgomery is true or false");
      return N.exportPoints(ctx, points.handle, first, n, fb, montgomery);
    },
    /** msm-batched-affine.ts:74-328 with safe additions */
    msm: (scalars, points, n, verbose = false, options) => msmCommon(scalars, points, n, verbose, options, 1, 0),
    /** msm-batched-affine.ts:574-586 */
    msmUnsafe: (scalars, points, n, verbose = false, options) => msmCommon(scalars, points, n, verbose, options, 0, 0),
  };
  if (!te) {
    /** parallel.ts:69-87 */
    Parallel.msmProjective = (scalars, points, n, options) =>
      msmCommon(scalars, points, n, true, Object.assign({}, options, { glv: 0 }), 1, 1);
  }

  curve.Parallel = Parallel;
  // "wasm memory" of the reference as far as its scripts touch it: memoryBytes.set(bytes, ptr) and field equality
  curve.Field = {
    sizeField: fb,
    memoryBytes: { set: (bytes, ptr) => { const [r, off] = space.find(ptr); stage(r, off, bytes, Math.floor((off + bytes.length) / recSize[r.kind])); } },
    /** field-arithmetic.ts:184-199 on staged canonical bytes: are the field elements at the two addresses equal? */
    isEqual(a, b) {
      const [ra, oa] = space.find(a), [rb, ob] = space.find(b);
      if (ra.host === null || rb.host === null) throw Error("Field.isEqual: nothing was written there");
      return ra.host.compare(rb.host, ob, ob + fb, oa, oa + fb) === 0;
    },
    local: { getPointers: (n) => Array.from({ length: n }, () => space.alloc(2 * fb, "field")), getPointer: (size) => space.alloc(size, "field") },
  };
  curve.Scalar = {
    sizeField: 32,
    memoryBytes: { set: (bytes, ptr) => { const [r, off] = space.find(ptr); stage(r, off, bytes, Math.floor((off + bytes.length) / 32)); } },
    /** Scalar.writeBigint(ptr, s): scripts/zprize23/submission-bls377.ts:95-102 */
    writeBigint(ptr, s) {
      if (s < 0n || s >= params.order) throw Error("scalar out of range");
      const [r, off] = space.find(ptr);
      stage(r, off, bigintToBytes(s, 32), off / 32 + 1);
    },
    modulus: params.order,
    sizeInBits: (params.order - 1n).toString(2).length,
    readBigint: (arr, i = 0) => bytesToBigint(N.downloadScalars(ctx, arr.handle, i, 1), 0, 32),
    toBigints(arr, first = 0, count = arr.n - first) {
      const b = N.downloadScalars(ctx, arr.handle, first, count);
      return Array.from({ length: count }, (_, i) => bytesToBigint(b, 32 * i, 32));
    },
    fromBigints: (scalars) => Parallel.scalarsFromBytes(Buffer.concat(scalars.map((s) => bigintToBytes(s, 32)))),
  };
  curve.Affine = {
    size: 2 * fb,
    /** curve-affine.ts:220-233; accepts an MSM result, or a pointer Projective.toAffine wrote to */
    toBigint: (p) => (typeof p === "number" ? space.find(p)[0].result : p),
    /** curve-affine.ts:290-308: canonical bigint points behind a pointer (isZero -> infinity flag) */
    writeBigints(ptr, points) {
      const [r, off] = space.find(ptr);
      const first = off / (2 * fb);
      if (r.inf === null) r.inf = new Uint8Array(Math.floor(r.size / (2 * fb)));
      points.forEach((p, i) => {
        r.inf[first + i] = p.isZero ? 1 : 0;
        stage(r, off + i * 2 * fb, Buffer.concat([bigintToBytes(p.isZero ? 0n : p.x, fb), bigintToBytes(p.isZero ? 0n : p.y, fb)]), first + i + 1);
      });
      return ptr;
    },
    toBigints(arr, first = 0, count = arr.n - first) {
      const b = N.downloadPoints(ctx, arr.handle, first, count, fb);
      return Array.from({ length: count }, (_, i) => {
        let zero = !te;
        for (let j = 0; j < 2 * fb && zero; j++) zero = b[2 * fb * i + j] === 0;
        return decodePoint(b, 2 * fb * i, zero);
      });
    },
    fromBigints(points) {
      const data = Buffer.concat(points.map((p) => Buffer.concat([bigintToBytes(p.x, fb), bigintToBytes(p.y, fb)])));
      const inf = Buffer.from(points.map((p) => (p.isZero ? 1 : 0)));
      return Parallel.pointsFromBytes(data, points.length, inf.some((v) => v) ? inf : null);
    },
  };
  // the reference converts the projective result with Projective.toAffine(scratch, affPtr, result)
  // (scripts/msm-weierstrass.ts:90-92); results here are already canonical affine points
  curve.Projective = {
    toAffine(_scratch, affPtr, result) {
      if (typeof affPtr === "number") space.find(affPtr)[0].result = result;
      return result;
    },
    toBigint: (result) => result,
  };
  curve.Curve = { toBigint: (result) => result };
  curve.pointAdd = (a, b) => {
    const enc = (p) => (p.isZero ? null : Buffer.concat([bigintToBytes(p.x, fb), bigintToBytes(p.y, fb)]));
    const r = N.pointAdd(params.curveId, enc(a), enc(b), fb);
    return decodePoint(r.xy, 0, r.isInf);
  };
  curve.close = () => N.destroy(ctx);
  return curve;
}

export const Weierstraß = { create: async (params) => createCurve(params, "weierstrass") };
export const Weierstrass = Weierstraß;
export const TwistedEdwards = { create: async (params) => createCurve(params, "twisted-edwards") };
