// Per-point scalar multiplication from the JavaScript host (Parallel.mulPoints over napi mulPoints, msmz_points_mul).
//   node js/scripts/msm-mul-points.mjs FIXTURE.json
//   -> one JSON line {plain, added, broadcast, fold, refused, msm}
// FIXTURE.json (tests/golden/points_mul_js_fixture.json, written by tests/golden/make_points_mul_fixture.py) holds n
// rows of BLS12-377: scalars, points and addends as decimal strings, and one scalar u.  plain: [s_i] P_i; added:
// [s_i] P_i + Q_i; broadcast: [u] P_i + Q_i; fold: the IPA fold of the points' halves, P_lo,i + [u] P_hi,i, with the ONE
// array as both operands -- each as [{x, y, isZero}, ...].  refused: a scalar >= the group order and a range beyond the
// set throw before the device; msm: the result is an ordinary point set (an MSM with scalars 1, 0, 0, ... over `added`
// returns its point 0).
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
  const u = BigInt(fx.u);
  const show = (arr) => Affine.toBigints(arr).map((p) => ({ x: p.x.toString(), y: p.y.toString(), isZero: !!p.isZero }));
  const plainArr = await Parallel.mulPoints(scalars, points);
  const addedArr = await Parallel.mulPoints(scalars, points, n, { addend });
  const broadcastArr = await Parallel.mulPoints(u, points, n, { addend });
  const half = n >> 1;
  const foldArr = await Parallel.mulPoints(u, points, half, { addend: points, firstPoint: half });
  let refused = 0;
  for (const bad of [() => Parallel.mulPoints(curveParams.order, points), () => Parallel.mulPoints(scalars, points, n, { firstPoint: 1 }),
                     () => Parallel.mulPoints(points, points)]) {
    try {
      await bad();
    } catch (e) {
      if (/mulPoints/.test(e.message)) refused++;
    }
  }
  const s = Buffer.alloc(32 * n);
  s[0] = 1;
  const r = (await Parallel.msm(s, addedArr, n)).result;
  const p0 = Affine.toBigints(addedArr, 0, 1)[0];
  console.log(JSON.stringify({ plain: show(plainArr), added: show(addedArr), broadcast: show(broadcastArr), fold: show(foldArr),
                               refused: refused === 3, msm: r.x === p0.x && r.y === p0.y && !!r.isZero === !!p0.isZero }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
