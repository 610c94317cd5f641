// Exports from the JavaScript host: Parallel.scalarsToBytes(scalars, {first, n, width, montgomery}) and
// Parallel.pointsToBytes(points, {first, n, montgomery}) (msmz_export_scalars / msmz_export_points on the host route,
// through napi/msmz_napi.c exportScalars / exportPoints).
//   node js/scripts/msm-export.mjs tests/golden/export_js_fixture.json
//   -> one JSON line {canonical, narrow, montgomery, range, pointsCanonical, pointsMontgomery, isInf, pointsRange,
//                     roundTrip, tooWide, refusedArgs, after}
// canonical / narrow / montgomery: the scalar records, hex (narrow: the 64-bit scalars at width 8); range: records
// [5, 5 + 20) of the Montgomery form alone; pointsCanonical / pointsMontgomery / isInf / pointsRange: the same for the
// points; roundTrip: the Montgomery records, read back by scalarsFromBytes / pointsFromBytes, download as the inputs;
// tooWide: the status code a full-length scalar throws with at width 8 ("6"); refusedArgs: the host refuses bad
// arguments before any call; after: a good call after the refused ones is still right.
import { readFileSync } from "fs";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const n = fx.n, fb = fx.feBytes;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Affine, Scalar } = Curve;
  const hex = (b) => Buffer.from(b).toString("hex");
  const want = fx.points.map((q) => ({ x: BigInt(q.x), y: BigInt(q.y), isZero: q.isZero }));
  const scalars = await Scalar.fromBigints(fx.scalars.map(BigInt));
  const scalars64 = await Scalar.fromBigints(fx.scalars64.map(BigInt));
  const points = await Affine.fromBigints(want);
  const out = { refusedArgs: 0 };
  out.canonical = hex(await Parallel.scalarsToBytes(scalars));
  out.narrow = hex(await Parallel.scalarsToBytes(scalars64, { width: 8 }));
  const mont = await Parallel.scalarsToBytes(scalars, { montgomery: true });
  out.montgomery = hex(mont);
  out.range = hex(await Parallel.scalarsToBytes(scalars, { first: 5, n: 20, montgomery: true }));
  const pc = await Parallel.pointsToBytes(points);
  out.pointsCanonical = hex(pc.records);
  out.isInf = Array.from(pc.isInf);
  const pm = await Parallel.pointsToBytes(points, { montgomery: true });
  out.pointsMontgomery = hex(pm.records);
  out.pointsRange = hex((await Parallel.pointsToBytes(points, { first: 5, n: 20, montgomery: true })).records);
  const s2 = await Parallel.scalarsFromBytes(mont, n, { montgomery: true });
  const p2 = await Parallel.pointsFromBytes(pm.records, n, { montgomery: true, isInf: pm.isInf });
  const backS = Scalar.toBigints(s2), backP = Affine.toBigints(p2);
  out.roundTrip = backS.every((v, i) => v === BigInt(fx.scalars[i])) &&
    backP.every((q, i) => q.isZero === want[i].isZero && (q.isZero || (q.x === want[i].x && q.y === want[i].y)));
  try { await Parallel.scalarsToBytes(scalars, { width: 8 }); out.tooWide = "accepted"; } catch (e) { out.tooWide = e.code; }
  for (const f of [() => Parallel.scalarsToBytes(points), () => Parallel.pointsToBytes(scalars), () => Parallel.scalarsToBytes(scalars, { first: n }),
                   () => Parallel.scalarsToBytes(scalars, { n: n + 1 }), () => Parallel.scalarsToBytes(scalars, { first: 1, n }),
                   () => Parallel.scalarsToBytes(scalars, { n: 0 }), () => Parallel.scalarsToBytes(scalars, { width: 6 }),
                   () => Parallel.scalarsToBytes(scalars, { width: 8, montgomery: true }), () => Parallel.scalarsToBytes(scalars, { montgomery: 1 }),
                   () => Parallel.pointsToBytes(points, { first: -1 }), () => Parallel.pointsToBytes(points, { n: n + 1 }),
                   () => Parallel.pointsToBytes(points, { montgomery: "yes" })]) {
    try { await f(); } catch (e) { out.refusedArgs++; }
  }
  out.after = hex(await Parallel.scalarsToBytes(scalars, { first: 0, n: 4 })) === out.canonical.slice(0, 2 * 32 * 4);
  console.log(JSON.stringify(out));
  Curve.close();
}

main().catch((e) => { console.error(e); process.exit(1); });
