// The argument checks of js/parallel.mjs as a table of calls, good and bad, on BLS12-377 with 16 random points and 16
// random scalars: what each call of Parallel.* throws, or that it runs.
//   node js/scripts/msm-args.mjs
//   -> one JSON line: [[label, threw, constructor name of the error, message], ...]
// tests/golden/js_args_parity.json is this line recorded before the host bindings were restructured;
// tests/test_js_args.py runs the script on the code under test and compares.  Every accepted call really runs, so
// every accepted call stays at n <= 16.
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

function le(x, len) {
  const out = Buffer.alloc(len);
  for (let i = 0; i < len; i++) { out[i] = Number(x & 0xffn); x >>= 8n; }
  return out;
}

async function main() {
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel: P, Scalar, Affine, Field } = Curve;
  const q = curveParams.order, fb = curveParams.feBytes;
  const pts = await P.randomPointsFast(16), x = await P.randomScalars(16), y = await P.randomScalars(8, { seed: 5n });
  const pts8 = await P.randomPointsFast(8, { seed: 5n });
  const alias = (a) => a.constructor.make(a.curve, a.handle, a.n, a.kind);   // a second object for the same handle
  const x2 = alias(x);
  const two = Affine.toBigints(pts, 0, 2);
  const pbytes = Buffer.concat(two.map((p) => Buffer.concat([le(p.x, fb), le(p.y, fb)])));
  const sbytes = Buffer.concat(Scalar.toBigints(x, 0, 4).map((s) => le(s, 32)));
  const rows = [];
  const t = async (label, fn) => {
    try {
      await fn();
      rows.push([label, false, "", ""]);
    } catch (e) {
      rows.push([label, true, e.constructor.name, String(e.message)]);
    }
  };
  const badFirst = [-1, 1.5, "1", true, null];
  const badN = [0, -1, 1.5, "4", true, 17, 2 ** 32];

  // ---- mulPoints(scalars, points, n, {addend, firstPoint, firstScalar, firstAddend})
  await t("mul ok", () => P.mulPoints(x, pts));
  await t("mul ok broadcast", () => P.mulPoints(5n, pts, 4));
  await t("mul ok fold", () => P.mulPoints(x, pts, 8, { addend: pts, firstPoint: 8 }));
  await t("mul ok firstScalar", () => P.mulPoints(x, pts, undefined, { firstScalar: 8, addend: pts8 }));
  for (const [k, v] of Object.entries({ scalars: x, nul: null, num: 7, undef: undefined }))
    await t(`mul points=${k}`, () => P.mulPoints(x, v));
  for (const [k, v] of Object.entries({ scalars: x, num: 7 })) await t(`mul addend=${k}`, () => P.mulPoints(x, pts, 4, { addend: v }));
  for (const [k, v] of Object.entries({ points: pts, num: 5, nul: null, str: "5" })) await t(`mul scalars=${k}`, () => P.mulPoints(v, pts));
  await t("mul scalar=q", () => P.mulPoints(q, pts));
  await t("mul scalar=-1", () => P.mulPoints(-1n, pts));
  for (const name of ["firstPoint", "firstScalar", "firstAddend"])
    for (const v of [...badFirst, 16, 8, 15]) await t(`mul ${name}=${String(v)}`, () => P.mulPoints(x, pts, 1, { addend: pts8, [name]: v }));
  await t("mul firstScalar without", () => P.mulPoints(5n, pts, 4, { firstScalar: 1 }));
  await t("mul firstAddend without", () => P.mulPoints(x, pts, 4, { firstAddend: 1 }));
  for (const v of badN) await t(`mul n=${String(v)}`, () => P.mulPoints(x, pts, v));
  await t("mul n=9 addend8", () => P.mulPoints(x, pts, 9, { addend: pts8 }));
  await t("mul n=9 firstPoint=8", () => P.mulPoints(x, pts, 9, { firstPoint: 8 }));
  await t("mul double points+scalar", () => P.mulPoints(q, x));
  await t("mul double scalar+first", () => P.mulPoints(q, pts, 0, { firstPoint: -1 }));
  await t("mul double firsts", () => P.mulPoints(x, pts, 0, { firstScalar: 16, firstPoint: 16 }));
  await t("mul double n+first", () => P.mulPoints(x, pts, 0, { firstAddend: 1 }));

  // ---- combineScalars(a, x, b, y, n, {firstX, firstY, out, firstOut, firstA, firstB})
  await t("comb ok", () => P.combineScalars(1n, x));
  await t("comb ok two", () => P.combineScalars(2n, x, 3n, y));
  await t("comb ok arrays", () => P.combineScalars(y, x, x, y, 4, { firstX: 1, firstY: 2, firstA: 3, firstB: 4 }));
  for (const [k, v] of Object.entries({ points: pts, nul: null, num: 7 })) {
    await t(`comb x=${k}`, () => P.combineScalars(1n, v));
    await t(`comb a=${k}`, () => P.combineScalars(v, x));
    if (v !== null) await t(`comb y=${k}`, () => P.combineScalars(1n, x, 1n, v));
    if (v !== null) await t(`comb out=${k}`, () => P.combineScalars(1n, x, null, null, 4, { out: v }));
    if (v !== null) await t(`comb b=${k}`, () => P.combineScalars(1n, x, v, y));
  }
  await t("comb b without y", () => P.combineScalars(1n, x, 1n));
  await t("comb y without b", () => P.combineScalars(1n, x, null, y));
  await t("comb a=q", () => P.combineScalars(q, x));
  await t("comb b=-1", () => P.combineScalars(1n, x, -1n, y));
  for (const [name, size] of [["firstX", 16], ["firstY", 8], ["firstA", 8], ["firstB", 16], ["firstOut", 16]])
    for (const v of [...badFirst, size, size - 1])
      await t(`comb ${name}=${String(v)}`, () => P.combineScalars(y, x, x, y, 1, { out: x2, [name]: v }));
  for (const name of ["firstY", "firstA", "firstB", "firstOut"]) await t(`comb ${name} without`, () => P.combineScalars(1n, x, null, null, 4, { [name]: 1 }));
  for (const v of badN) await t(`comb n=${String(v)}`, () => P.combineScalars(1n, x, null, null, v));
  await t("comb n=9 y8", () => P.combineScalars(1n, x, 1n, y, 9));
  await t("comb n=5 firstY=4", () => P.combineScalars(1n, x, 1n, y, 5, { firstY: 4 }));
  for (const [k, o] of [["same", x], ["alias", x2]])
    for (const d of [0, 1, 3, 4]) {
      await t(`comb out=${k} x d=${d}`, () => P.combineScalars(1n, x, null, null, 4, { out: o, firstOut: d }));
      await t(`comb out=${k} y d=-${d}`, () => P.combineScalars(1n, y, 2n, x, 4, { firstY: 8, out: o, firstOut: 8 - d }));
      await t(`comb out=${k} a d=${d}`, () => P.combineScalars(x, y, null, null, 4, { firstA: 2, out: o, firstOut: 2 + d }));
    }
  await t("comb double x+coeff", () => P.combineScalars(q, pts));
  await t("comb double coeffs", () => P.combineScalars(q, x, q + 1n, y));
  await t("comb double coeff+first", () => P.combineScalars(q, x, null, null, 0, { firstX: -1 }));
  await t("comb double firsts", () => P.combineScalars(1n, x, null, null, 0, { firstA: 1, firstX: 16 }));
  await t("comb double n+overlap", () => P.combineScalars(1n, x, null, null, 17, { out: x, firstOut: 1 }));
  await t("comb double fit+overlap", () => P.combineScalars(1n, x, 1n, y, 9, { out: x, firstOut: 1 }));

  // ---- innerProduct(x, y, n, {firstX, firstY})
  await t("dot ok sum", () => P.innerProduct(x));
  await t("dot ok", () => P.innerProduct(x, y));
  await t("dot ok self", () => P.innerProduct(x, x, 8, { firstY: 8 }));
  await t("dot x=points", () => P.innerProduct(pts));
  await t("dot y=points", () => P.innerProduct(x, pts));
  await t("dot x=null", () => P.innerProduct(null));
  for (const name of ["firstX", "firstY"])
    for (const v of [...badFirst, 16, 8, 7]) await t(`dot ${name}=${String(v)}`, () => P.innerProduct(x, y, 1, { [name]: v }));
  await t("dot firstY without", () => P.innerProduct(x, null, 4, { firstY: 1 }));
  for (const v of badN) await t(`dot n=${String(v)}`, () => P.innerProduct(x, null, v));
  await t("dot n=9 y8", () => P.innerProduct(x, y, 9));
  await t("dot double", () => P.innerProduct(x, y, 0, { firstX: 16, firstY: 8 }));

  // ---- scalarPowers(ratio, n, base)
  await t("pow ok", () => P.scalarPowers(2n, 4));
  await t("pow ok base", () => P.scalarPowers(0n, 16, 3n));
  for (const [k, v] of Object.entries({ num: 2, str: "2", nul: null, q, neg: -1n })) {
    await t(`pow ratio=${k}`, () => P.scalarPowers(v, 4));
    await t(`pow base=${k}`, () => P.scalarPowers(2n, 4, v));
  }
  for (const v of [0, -1, 1.5, "4", true, 2 ** 32, undefined]) await t(`pow n=${String(v)}`, () => P.scalarPowers(2n, v));
  await t("pow double", () => P.scalarPowers(q, 0, 2));

  // ---- scalarRecurrence(a, b, n, {init, reverse, exclusive, firstA, firstB, out, firstOut}) and its wrappers
  await t("rec ok sums", () => P.scalarRecurrence(null, x));
  await t("rec ok products", () => P.scalarRecurrence(x, null, 8, { exclusive: true }));
  await t("rec ok broadcast", () => P.scalarRecurrence(3n, y, undefined, { init: 0n, reverse: true, exclusive: true }));
  await t("rec ok general", () => P.scalarRecurrence(x, y, 4, { firstA: 4, firstB: 2, init: q - 1n }));
  await t("rec ok powers", () => P.scalarRecurrence(3n, null, 5));
  await t("rec nothing", () => P.scalarRecurrence(null, null, 4));
  for (const [k, v] of Object.entries({ points: pts, num: 5, str: "5" })) {
    await t(`rec a=${k}`, () => P.scalarRecurrence(v, y));
    await t(`rec b=${k}`, () => P.scalarRecurrence(x, v));
    await t(`rec out=${k}`, () => P.scalarRecurrence(x, y, 4, { out: v }));
    await t(`rec init=${k}`, () => P.scalarRecurrence(x, y, 4, { init: v }));
  }
  await t("rec b=bigint", () => P.scalarRecurrence(x, 3n));
  await t("rec a=q", () => P.scalarRecurrence(q, y));
  await t("rec init=q", () => P.scalarRecurrence(x, y, 4, { init: q }));
  await t("rec init=-1", () => P.scalarRecurrence(x, y, 4, { init: -1n }));
  for (const [name, size] of [["firstA", 16], ["firstB", 8], ["firstOut", 16]])
    for (const v of [...badFirst, size, size - 1]) await t(`rec ${name}=${String(v)}`, () => P.scalarRecurrence(x, y, 1, { out: x2, [name]: v }));
  await t("rec firstA without", () => P.scalarRecurrence(3n, y, 4, { firstA: 1 }));
  await t("rec firstB without", () => P.scalarRecurrence(x, null, 4, { firstB: 1 }));
  await t("rec firstOut without", () => P.scalarRecurrence(x, null, 4, { firstOut: 1 }));
  await t("rec no length", () => P.scalarRecurrence(3n, null));
  for (const v of badN) await t(`rec n=${String(v)}`, () => P.scalarRecurrence(x, null, v));
  await t("rec n=9 b8", () => P.scalarRecurrence(x, y, 9));
  for (const [k, o] of [["same", x], ["alias", x2]])
    for (const d of [0, 1, 3, 4]) {
      await t(`rec out=${k} a d=${d}`, () => P.scalarRecurrence(x, null, 4, { out: o, firstOut: d }));
      await t(`rec out=${k} b d=-${d}`, () => P.scalarRecurrence(null, x, 4, { firstB: 8, out: o, firstOut: 8 - d }));
    }
  await t("rec double types", () => P.scalarRecurrence(pts, pts));
  await t("rec double range+first", () => P.scalarRecurrence(q, y, 0, { firstA: -1 }));
  await t("rec double n+overlap", () => P.scalarRecurrence(x, null, 17, { out: x, firstOut: 1 }));
  await t("prefixSums ok", () => P.prefixSums(y));
  await t("prefixSums first=1 n=8", () => P.prefixSums(y, 8, { first: 1 }));
  await t("prefixProducts ok in place", () => P.prefixProducts(y, 4, { out: y }));
  await t("prefixProducts overlap", () => P.prefixProducts(y, 4, { out: y, firstOut: 1 }));
  await t("prefixProducts points", () => P.prefixProducts(pts));
  await t("divideByLinear ok", () => P.divideByLinear(y, 5n));
  await t("divideByLinear z=num", () => P.divideByLinear(y, 5));
  await t("divideByLinear p=points", () => P.divideByLinear(pts, 5n));
  await t("divideByLinear double", () => P.divideByLinear(pts, 5));
  await t("divideByLinear z=q", () => P.divideByLinear(y, q));
  await t("divideByLinear n=9", () => P.divideByLinear(y, 5n, 9));

  // ---- invertScalars(x, n, {first, out, firstOut})
  await t("inv ok", () => P.invertScalars(x));
  await t("inv ok in place", () => P.invertScalars(y, 4, { out: y }));
  await t("inv ok apart", () => P.invertScalars(y, 4, { first: 4, out: x, firstOut: 12 }));
  for (const [k, v] of Object.entries({ points: pts, nul: null, num: 5 })) {
    await t(`inv x=${k}`, () => P.invertScalars(v));
    if (v !== null) await t(`inv out=${k}`, () => P.invertScalars(x, 4, { out: v }));
  }
  for (const [name, size] of [["first", 16], ["firstOut", 8]])
    for (const v of [...badFirst, size, size - 1]) await t(`inv ${name}=${String(v)}`, () => P.invertScalars(x, 1, { out: y, [name]: v }));
  await t("inv firstOut without", () => P.invertScalars(x, 4, { firstOut: 1 }));
  for (const v of badN) await t(`inv n=${String(v)}`, () => P.invertScalars(x, v));
  await t("inv n=9 out8", () => P.invertScalars(x, 9, { out: y }));
  for (const [k, o] of [["same", x], ["alias", x2]])
    for (const d of [0, 1, 3, 4]) await t(`inv out=${k} d=${d}`, () => P.invertScalars(x, 4, { out: o, firstOut: d }));
  await t("inv double", () => P.invertScalars(x, 0, { first: 16 }));
  await t("inv double n+overlap", () => P.invertScalars(x, 17, { out: x, firstOut: 1 }));

  // ---- checkPoints(points, n, {subgroup, first, verdicts})
  await t("check ok", () => P.checkPoints(pts));
  await t("check ok range", () => P.checkPoints(pts, 4, { first: 12, subgroup: false, verdicts: true }));
  for (const [k, v] of Object.entries({ scalars: x, nul: null, num: 5 })) await t(`check points=${k}`, () => P.checkPoints(v));
  for (const v of [...badFirst, 16, 17]) await t(`check first=${String(v)}`, () => P.checkPoints(pts, 1, { first: v }));
  for (const v of badN) await t(`check n=${String(v)}`, () => P.checkPoints(pts, v));
  await t("check n=5 first=12", () => P.checkPoints(pts, 5, { first: 12 }));
  await t("check double", () => P.checkPoints(pts, 0, { first: 16 }));

  // ---- precomputePoints(points, n, options, factor)
  await t("pre ok", () => P.precomputePoints(pts, 16));
  await t("pre ok c factor", () => P.precomputePoints(pts, 8, { c: 8, glv: 0 }, 2));
  await t("pre ok scalarBits", () => P.precomputePoints(pts, 16, { glv: 1, scalarBits: 64 }, 0));
  for (const [k, v] of Object.entries({ scalars: x, nul: null, num: 5 })) await t(`pre points=${k}`, () => P.precomputePoints(v, 4));
  for (const v of [0, -1, 1.5, "4", true, 17, undefined]) await t(`pre n=${String(v)}`, () => P.precomputePoints(pts, v));
  for (const v of [1, -1, 1.5, "2", true, 2 ** 32, null]) await t(`pre factor=${String(v)}`, () => P.precomputePoints(pts, 8, {}, v));
  for (const v of [257, -1, 1.5, "64", true]) await t(`pre scalarBits=${String(v)}`, () => P.precomputePoints(pts, 8, { scalarBits: v }));
  await t("pre double n+factor", () => P.precomputePoints(pts, 0, { scalarBits: 300 }, 1));
  await t("pre double factor+bits", () => P.precomputePoints(pts, 8, { scalarBits: 300 }, 1));
  const pre = await P.precomputePoints(pts, 16);
  await t("pre of precomputed", () => P.precomputePoints(pre, 8));
  await t("mul points=precomputed", () => P.mulPoints(x, pre));
  await t("check points=precomputed", () => P.checkPoints(pre));

  // ---- msmSegments(scalars, points, segments, options)
  await t("seg ok", () => P.msmSegments(x, pts, [[0, 0, 16]]));
  await t("seg ok two", () => P.msmSegmentsUnsafe(x, pts, [[8, 0, 8], [0, 8, 8], [3, 3, 1]]));
  await t("seg ok precomputed", () => P.msmSegments(x, pre, [[0, 0, 16]], { scalarBits: 0 }));
  for (const [k, v] of Object.entries({ scalars: x, nul: null, num: 5 })) await t(`seg points=${k}`, () => P.msmSegments(x, v, [[0, 0, 1]]));
  for (const [k, v] of Object.entries({ points: pts, nul: null, buf: sbytes })) await t(`seg scalars=${k}`, () => P.msmSegments(v, pts, [[0, 0, 1]]));
  const badSegs = { empty: [], str: "abc", nul: null, num: 5, pair: [[0, 0]], four: [[0, 0, 1, 1]], flat: [0, 0, 1], n0: [[0, 0, 0]], n17: [[0, 0, 17]],
                    neg: [[-1, 0, 1]], frac: [[0, 1.5, 1]], strn: [[0, 0, "1"]], p1: [[1, 0, 16]], s1: [[0, 1, 16]], second: [[0, 0, 1], [0, 16, 1]] };
  for (const [k, v] of Object.entries(badSegs)) await t(`seg segments=${k}`, () => P.msmSegments(x, pts, v));
  for (const v of [257, -1, 1.5, "64"]) await t(`seg scalarBits=${String(v)}`, () => P.msmSegments(x, pts, [[0, 0, 16]], { scalarBits: v }));
  await t("seg double bits+points", () => P.msmSegments(x, x, [], { scalarBits: 300 }));
  await t("seg double points+scalars", () => P.msmSegments(pts, x, []));
  await t("seg double scalars+segments", () => P.msmSegments(pts, pts, []));

  // ---- msmBatch(scalarsList, points, n, options)
  const vec = sbytes;   // 4 scalars
  await t("batch ok resident", () => P.msmBatch(x, pts, 8));
  await t("batch ok batch=2", () => P.msmBatchUnsafe(x, pts, 4, { batch: 2 }));
  await t("batch ok host", () => P.msmBatch([vec, vec, vec], pts, 4));
  await t("batch ok precomputed", () => P.msmBatch(x, pre, 16, { scalarBits: 256 }));
  for (const v of [0, -1, 17, undefined, "4"]) await t(`batch n=${String(v)}`, () => P.msmBatch(x, pts, v));
  for (const v of [0, -1, 5]) await t(`batch batch=${String(v)}`, () => P.msmBatch(x, pts, 4, { batch: v }));
  const badLists = { empty: [], str: "abc", nul: null, resident: [x], pointer: [5], unequal: [vec, vec.subarray(0, 64)], short: [vec, vec] };
  for (const [k, v] of Object.entries(badLists)) await t(`batch list=${k}`, () => P.msmBatch(v, pts, k === "short" ? 5 : 2));
  for (const v of [257, -1, 1.5, "64"]) await t(`batch scalarBits=${String(v)}`, () => P.msmBatch(x, pts, 8, { scalarBits: v }));
  await t("batch double bits+n", () => P.msmBatch(x, pts, 0, { scalarBits: 300 }));
  await t("batch double n+list", () => P.msmBatch([], pts, 17));

  // ---- msm(scalars, points, n, verbose, options): the options only
  await t("msm ok", () => P.msm(x, pts, 16));
  await t("msm ok host", () => P.msmUnsafe(sbytes, pts, 4, true, { c: 4, glv: 0, scalarBits: 253 }));
  for (const v of [257, -1, 1.5, "64"]) await t(`msm scalarBits=${String(v)}`, () => P.msm(x, pts, 16, false, { scalarBits: v }));

  // ---- pointsFromBytes: (bytes, n, isInf | {montgomery, isInf}) and (ptr, inputPtr, n)
  await t("pfb ok", () => P.pointsFromBytes(pbytes));
  await t("pfb ok n=1", () => P.pointsFromBytes(pbytes, 1));
  await t("pfb ok isInf", () => P.pointsFromBytes(pbytes, 2, new Uint8Array([0, 1])));
  await t("pfb ok options", () => P.pointsFromBytes(pbytes, 2, { isInf: [1, 0] }));
  await t("pfb short", () => P.pointsFromBytes(pbytes.subarray(0, 95)));
  await t("pfb n=3", () => P.pointsFromBytes(pbytes, 3));
  await t("pfb n=0", () => P.pointsFromBytes(pbytes, 0));
  await t("pfb n=-1", () => P.pointsFromBytes(pbytes, -1));
  await t("pfb isInf short", () => P.pointsFromBytes(pbytes, 2, new Uint8Array(1)));
  await t("pfb isInf short options", () => P.pointsFromBytes(pbytes, 2, { montgomery: true, isInf: [1] }));
  await t("pfb empty", () => P.pointsFromBytes(Buffer.alloc(0)));
  const pp = await P.getPointer(2 * 2 * fb), pin = await P.getPointer(2 * 2 * fb), pempty = await P.getPointer(2 * 2 * fb);
  Field.memoryBytes.set(pbytes, pin);
  await t("pfb ptr ok", () => P.pointsFromBytes(pp, pin, 2));
  await t("pfb ptr ok again", () => P.pointsFromBytes(pp, pin, 1));
  await t("pfb ptr offset", () => P.pointsFromBytes(pp + 8, pin, 2));
  await t("pfb ptr nothing written", () => P.pointsFromBytes(pp, pempty, 2));
  await t("pfb ptr beyond", () => P.pointsFromBytes(pp, pin, 3));
  await t("pfb ptr input offset beyond", () => P.pointsFromBytes(pp, pin + 2 * fb, 2));
  await t("pfb ptr unknown", () => P.pointsFromBytes(12345, pin, 2));
  await t("pfb ptr unknown input", () => P.pointsFromBytes(pp, 12345, 2));

  // ---- scalarsFromBytes: (bytes, n, {width, montgomery}) and (ptr, inputPtr, n)
  await t("sfb ok", () => P.scalarsFromBytes(sbytes));
  await t("sfb ok n=2", () => P.scalarsFromBytes(sbytes, 2));
  await t("sfb ok width=8", () => P.scalarsFromBytes(sbytes.subarray(0, 32), undefined, { width: 8 }));
  await t("sfb ok width=32", () => P.scalarsFromBytes(sbytes, 4, { width: 32 }));
  await t("sfb short", () => P.scalarsFromBytes(sbytes.subarray(0, 31)));
  await t("sfb n=5", () => P.scalarsFromBytes(sbytes, 5));
  await t("sfb n=0", () => P.scalarsFromBytes(sbytes, 0));
  for (const v of [6, 36, 0, "8", true]) await t(`sfb width=${String(v)}`, () => P.scalarsFromBytes(sbytes, 2, { width: v }));
  await t("sfb montgomery width=8", () => P.scalarsFromBytes(sbytes, 2, { width: 8, montgomery: true }));
  await t("sfb width=8 n=17", () => P.scalarsFromBytes(sbytes, 17, { width: 8 }));
  await t("sfb double width+n", () => P.scalarsFromBytes(sbytes, 0, { width: 6 }));
  const sp = await P.getScalarPointer(4 * 32), sin = await P.getScalarPointer(4 * 32), sempty = await P.getScalarPointer(4 * 32);
  Scalar.memoryBytes.set(sbytes, sin);
  await t("sfb ptr ok", () => P.scalarsFromBytes(sp, sin, 4));
  await t("sfb ptr ok again", () => P.scalarsFromBytes(sp, sin + 32, 3));
  await t("sfb ptr offset", () => P.scalarsFromBytes(sp + 32, sin, 4));
  await t("sfb ptr nothing written", () => P.scalarsFromBytes(sp, sempty, 4));
  await t("sfb ptr beyond", () => P.scalarsFromBytes(sp, sin, 5));
  await t("sfb ptr unknown", () => P.scalarsFromBytes(12345, sin, 4));
  await t("msm ok pointers", () => P.msmUnsafe(sp, pp, 1));

  Curve.close();
  console.log(JSON.stringify(rows));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
