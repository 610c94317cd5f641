// Point-set validation from the JavaScript host (Parallel.checkPoints over napi checkPoints, msmz_check_points).
//   node js/scripts/msm-check-points.mjs LOG2N [PLANT.json]
//   -> one JSON line {good, curveOnly, planted, range, refused, msm}
// Points: randomPointsFast(2^LOG2N, seed 1) on BLS12-377.  good: the check of the generated set.  PLANT.json holds
// [{i, x, y}, ...] (decimal strings): the set is read back, those indices are overwritten and it is uploaded again;
// planted / curveOnly: its check with and without the subgroup test, with verdict bytes; range: the check of points
// [first, first + 64) around the first planted index; refused: a range beyond the set throws before the device; msm: the
// context still computes after all that (an MSM with scalars 1, 0, 0, ... returns point 0 of the generated set).
import { readFileSync } from "node:fs";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const args = process.argv.slice(2);
  const n = 1 << Number(args[0] || 12);
  const plant = args[1] ? JSON.parse(readFileSync(args[1], "utf8")) : [];
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Affine } = Curve;
  const points = await Parallel.randomPointsFast(n, { seed: 1n });
  const show = (r) => ({ ok: r.ok, offCurve: r.offCurve, offSubgroup: r.offSubgroup, firstBad: r.firstBad,
                         verdicts: r.verdicts ? Array.from(r.verdicts) : null });
  const good = show(await Parallel.checkPoints(points, n, { verdicts: true }));
  const pts = Affine.toBigints(points);
  for (const { i, x, y } of plant) pts[i] = { x: BigInt(x), y: BigInt(y), isZero: false };
  const bad = await Affine.fromBigints(pts);
  const planted = show(await Parallel.checkPoints(bad, undefined, { verdicts: true }));
  const curveOnly = show(await Parallel.checkPoints(bad, n, { subgroup: false, verdicts: true }));
  const first = plant.length ? Math.max(0, Math.min(...plant.map((p) => p.i)) - 10) : 0;
  const range = Object.assign(show(await Parallel.checkPoints(bad, Math.min(64, n - first), { first, verdicts: true })), { first });
  let refused = false;
  try {
    await Parallel.checkPoints(bad, n, { first: 1 });
  } catch (e) {
    refused = /checkPoints/.test(e.message);
  }
  const s = Buffer.alloc(32 * n);
  s[0] = 1;
  const r = (await Parallel.msm(s, points, n)).result;
  const p0 = Affine.toBigints(points, 0, 1)[0];
  console.log(JSON.stringify({ good, planted, curveOnly, range, refused, msm: r.x === p0.x && r.y === p0.y && !r.isZero }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
