// Per-point scalar multiplication with options from the JavaScript host (Parallel.mulPoints {scalarBits, subgroup} over
// napi mulPoints, msmz_points_mul_opts).
//   node js/scripts/msm-mul-points-opts.mjs FIXTURE.json
//   -> one JSON line {subgroup, broadcast, fold128, bounded64, same, refused, range}
// FIXTURE.json (tests/golden/points_mul_opts_js_fixture.json, written by tests/golden/make_points_mul_opts_fixture.py)
// holds n rows of BLS12-377 with every point in the prime-order subgroup: scalars, 64-bit scalars, points and addends as
// decimal strings, a scalar u and a 128-bit one.  subgroup: [s_i] P_i + Q_i under the vouch; broadcast: [u] P_i + Q_i
// under the vouch; fold128: the IPA fold of the points' halves with the 128-bit challenge, scalarBits = 128 and the
// vouch; bounded64: [t_i] P_i with scalarBits = 64 -- each as [{x, y, isZero}, ...].  same: the vouched results equal the
// plain calls'.  refused: a bad scalarBits, a non-boolean subgroup and a broadcast scalar beyond its bound throw before
// the device; range: resident scalars beyond their bound fail the call, and the next call works.
import { readFileSync } from "node:fs";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const n = fx.n;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Affine, Scalar } = Curve;
  const point = (p) => ({ x: BigInt(p.x), y: BigInt(p.y), isZero: !!p.isZero });
  const points = await Affine.fromBigints(fx.points.map(point));
  const addend = await Affine.fromBigints(fx.addend.map(point));
  const scalars = await Scalar.fromBigints(fx.scalars.map(BigInt));
  const scalars64 = await Scalar.fromBigints(fx.scalars64.map(BigInt));
  const u = BigInt(fx.u), u128 = BigInt(fx.u128);
  const show = (arr) => Affine.toBigints(arr).map((p) => ({ x: p.x.toString(), y: p.y.toString(), isZero: !!p.isZero }));
  const half = n >> 1;
  const subgroup = show(await Parallel.mulPoints(scalars, points, n, { addend, subgroup: true }));
  const broadcast = show(await Parallel.mulPoints(u, points, n, { addend, subgroup: true }));
  const fold128 = show(await Parallel.mulPoints(u128, points, half, { addend: points, firstPoint: half, scalarBits: 128, subgroup: true }));
  const bounded64 = show(await Parallel.mulPoints(scalars64, points, n, { scalarBits: 64 }));
  const plain = [show(await Parallel.mulPoints(scalars, points, n, { addend })), show(await Parallel.mulPoints(u, points, n, { addend }))];
  const same = JSON.stringify(plain) === JSON.stringify([subgroup, broadcast]);
  let refused = 0;
  for (const bad of [() => Parallel.mulPoints(scalars, points, n, { scalarBits: 257 }), () => Parallel.mulPoints(scalars, points, n, { scalarBits: 1.5 }),
                     () => Parallel.mulPoints(scalars, points, n, { subgroup: 1 }), () => Parallel.mulPoints(1n << 64n, points, n, { scalarBits: 64 })]) {
    try {
      await bad();
    } catch (e) {
      if (/mulPoints/.test(e.message)) refused++;
    }
  }
  let range = false;
  try {
    await Parallel.mulPoints(scalars, points, n, { scalarBits: 64, subgroup: true });
  } catch (e) {
    range = /msmz_points_mul_opts/.test(e.message);
  }
  range = range && JSON.stringify(show(await Parallel.mulPoints(scalars64, points, n, { scalarBits: 64, subgroup: true }))) === JSON.stringify(bounded64);
  console.log(JSON.stringify({ subgroup, broadcast, fold128, bounded64, same, refused: refused === 4, range }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
