// Recurrences and inversion over resident scalar arrays from the JavaScript host (Parallel.scalarRecurrence /
// prefixProducts / prefixSums / divideByLinear / invertScalars over napi scalarsRecurrence / scalarsInverse;
// msmz_scalars_recurrence / _inverse).
//   node js/scripts/msm-scalar-scan.mjs FIXTURE.json
//   -> one JSON line {sums, products, grand, quotient, value, general, inverse, zeros, inplace, refused}
// FIXTURE.json (tests/golden/scalar_scan_js_fixture.json, written by tests/golden/make_scalar_scan_fixture.py) holds n
// scalars x and y of BLS12-377 as decimal strings and the scalars z and init.  sums: the running sums of y and their
// total; products: the running products of x and the full product; grand: the exclusive products of x (entry 0 is 1);
// quotient, value: (y(X) - y(z)) / (X - z) and y(z); general: y_i = x_i y_(i-1) + y_i from init, in reverse, and its final
// value; inverse, zeros: x^-1 with 0 -> 0 and the zero count; inplace: a copy of x whose low half was inverted IN PLACE
// -- scalars as decimal strings, [vector, final value] pairs for the recurrences.  refused: a multiplier >= the group
// order, a range beyond the array, a partly overlapping destination and a call without operands throw before the device.
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
  const [z, init] = [BigInt(fx.z), BigInt(fx.init)];
  const show = ([arr, last]) => [Scalar.toBigints(arr).map((s) => s.toString()), last.toString()];
  const sums = show(await Parallel.prefixSums(y));
  const products = show(await Parallel.prefixProducts(x));
  const grand = show(await Parallel.prefixProducts(x, n, { exclusive: true }));
  const [quotient, value] = show(await Parallel.divideByLinear(y, z));
  const general = show(await Parallel.scalarRecurrence(x, y, n, { init, reverse: true }));
  const [inv, zeros] = await Parallel.invertScalars(x);
  const inverse = Scalar.toBigints(inv).map((s) => s.toString());
  const copy = await Parallel.combineScalars(1n, x);
  const [same] = await Parallel.invertScalars(copy, half, { out: copy });
  const inplace = Scalar.toBigints(copy).map((s) => s.toString());
  let refused = 0;
  for (const bad of [() => Parallel.scalarRecurrence(curveParams.order, y), () => Parallel.prefixSums(y, n, { first: 1 }),
                     () => Parallel.prefixProducts(copy, half, { out: copy, firstOut: 1 }), () => Parallel.scalarRecurrence(null, null, n),
                     () => Parallel.invertScalars(copy, half, { out: copy, firstOut: 1 }), () => Parallel.divideByLinear(y, 5)]) {
    try {
      await bad();
    } catch (e) {
      if (/scalarRecurrence|invertScalars|divideByLinear/.test(e.message)) refused++;
    }
  }
  console.log(JSON.stringify({ sums, products, grand, quotient, value, general, inverse, zeros, inplace,
                               refused: refused === 6 && same === copy }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
