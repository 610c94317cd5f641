// Arithmetic over resident scalar arrays from the JavaScript host (Parallel.combineScalars / innerProduct / scalarPowers
// over napi scalarsCombine / scalarsDot / scalarsPowers; msmz_scalars_combine / _dot / _powers).
//   node js/scripts/msm-scalar-ops.mjs FIXTURE.json
//   -> one JSON line {scaled, hadamard, combined, fold, dot, sum, cross, powers, refused}
// FIXTURE.json (tests/golden/scalar_ops_js_fixture.json, written by tests/golden/make_scalar_ops_fixture.py) holds n
// scalars x, y and c of BLS12-377 as decimal strings and the scalars a, b, z.  scaled: a x; hadamard: c . x; combined:
// c . x + b y; fold: x_lo + a x_hi written IN PLACE over the low half of a copy of x (the whole copy is returned); dot:
// <x, y>; sum: the sum of x; cross: <x_lo, y_hi>; powers: b z^i -- scalars as decimal strings.  refused: a coefficient
// >= the group order, a range beyond the array and a partly overlapping destination throw before the device.
import { readFileSync } from "node:fs";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const n = fx.n, half = n >> 1;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar } = Curve;
  const x = await Scalar.fromBigints(fx.x.map(BigInt));
  const y = await Scalar.fromBigints(fx.y.map(BigInt));
  const c = await Scalar.fromBigints(fx.c.map(BigInt));
  const [a, b, z] = [BigInt(fx.a), BigInt(fx.b), BigInt(fx.z)];
  const show = (arr) => Scalar.toBigints(arr).map((s) => s.toString());
  const scaled = show(await Parallel.combineScalars(a, x));
  const hadamard = show(await Parallel.combineScalars(c, x));
  const combined = show(await Parallel.combineScalars(c, x, b, y));
  const copy = await Parallel.combineScalars(1n, x);
  const same = await Parallel.combineScalars(1n, copy, a, copy, half, { firstY: half, out: copy });
  const fold = show(copy);
  const dot = (await Parallel.innerProduct(x, y)).toString();
  const sum = (await Parallel.innerProduct(x)).toString();
  const cross = (await Parallel.innerProduct(x, y, half, { firstY: half })).toString();
  const powers = show(await Parallel.scalarPowers(z, n, b));
  let refused = 0;
  for (const bad of [() => Parallel.combineScalars(curveParams.order, x), () => Parallel.combineScalars(a, x, null, null, n, { firstX: 1 }),
                     () => Parallel.combineScalars(1n, copy, a, copy, half, { firstY: half, out: copy, firstOut: 1 }),
                     () => Parallel.innerProduct(x, y, n, { firstY: 1 }), () => Parallel.scalarPowers(curveParams.order, 4)]) {
    try {
      await bad();
    } catch (e) {
      if (/combineScalars|innerProduct|scalarPowers/.test(e.message)) refused++;
    }
  }
  console.log(JSON.stringify({ scaled, hadamard, combined, fold, dot, sum, cross, powers, refused: refused === 5 && same === copy }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
