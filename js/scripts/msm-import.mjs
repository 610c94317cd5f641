// Narrow and Montgomery inputs from the JavaScript host: scalarsFromBytes(bytes, n, {width, montgomery}) and
// pointsFromBytes(bytes, n, {montgomery}) (the host-memory forms of msmz_import_*; N-API has no device pointers).
//   node js/scripts/msm-import.mjs LOG2N
//   -> one JSON line {plain, narrow, mont, scalarsEqual, pointsEqual, defaults, shortBuffer, refusedWidth, refusedMont,
//                      range, after}
// Points: randomPointsFast(2^LOG2N, seed 1); scalars: entry i = i + 1.  plain: msm over 32-byte canonical scalars; narrow:
// the same scalars as 8-byte records with scalarBits 64; mont: Montgomery scalars (v 2^256 mod q) over Montgomery points
// (v 2^(8 feBytes) mod p); scalarsEqual / pointsEqual: the imported sets read back as the canonical values; refusedWidth
// defaults: the byte route without n -- scalarsFromBytes(bytes), scalarsFromBytes(bytes, undefined, {width: 32}),
// Scalar.fromBigints(values) -- holds every scalar of the buffer, as before the options existed; shortBuffer: a buffer
// shorter than n scalars throws the host's own message; refusedWidth
// / refusedMont: width 6 and Montgomery at width 8 throw before the device; range: a Montgomery record equal to q
// throws; after: the same context then computes `plain` again.
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

const toBytes = (v, len) => {
  const b = Buffer.alloc(len);
  for (let i = 0; i < len; i++, v >>= 8n) b[i] = Number(v & 0xffn);
  return b;
};

async function main() {
  const n = 1 << Number(process.argv[2] || 10);
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar, Affine } = Curve;
  const q = Scalar.modulus, p = curveParams.modulus, fb = Affine.size / 2;
  const [points] = await Parallel.randomPointsFast(n, { seed: 1n });
  const pts = Affine.toBigints(points);
  const vals = Array.from({ length: n }, (_, i) => BigInt(i + 1));
  const wide = Buffer.concat(vals.map((v) => toBytes(v, 32)));
  const narrow = Buffer.concat(vals.map((v) => toBytes(v, 8)));
  const montS = Buffer.concat(vals.map((v) => toBytes((v << 256n) % q, 32)));
  const R = 1n << BigInt(8 * fb);
  const montP = Buffer.concat(pts.map((pt) => Buffer.concat([toBytes((pt.x * R) % p, fb), toBytes((pt.y * R) % p, fb)])));
  const show = (r) => ({ x: r.x.toString(), y: r.y.toString(), isZero: r.isZero });
  const s8 = await Parallel.scalarsFromBytes(narrow, n, { width: 8 });
  const sm = await Parallel.scalarsFromBytes(montS, n, { montgomery: true });
  const pm = await Parallel.pointsFromBytes(montP, n, { montgomery: true });
  const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);
  const scalarsEqual = same(Scalar.toBigints(s8), vals) && same(Scalar.toBigints(sm), vals);
  const back = Affine.toBigints(pm);
  const pointsEqual = back.length === n && back.every((pt, i) => pt.x === pts[i].x && pt.y === pts[i].y);
  let defaults = true, shortBuffer = false;
  for (const arr of [await Parallel.scalarsFromBytes(wide), await Parallel.scalarsFromBytes(wide, undefined, { width: 32 }),
                     await Parallel.scalarsFromBytes(wide, undefined, {}), await Scalar.fromBigints(vals)]) {
    defaults = defaults && arr.n === n && same(Scalar.toBigints(arr), vals);
    arr.free();
  }
  try { await Parallel.scalarsFromBytes(wide, n + 1); } catch (e) { shortBuffer = /scalarsFromBytes: \d+ bytes for \d+ scalars/.test(e.message); }
  const plain = (await Parallel.msm(wide, points, n)).result;
  const viaNarrow = (await Parallel.msm(s8, points, n, false, { scalarBits: 64 })).result;
  const viaMont = (await Parallel.msmUnsafe(sm, pm, n)).result;
  let refusedWidth = false, refusedMont = false, range = false;
  try { await Parallel.scalarsFromBytes(narrow, n, { width: 6 }); } catch (e) { refusedWidth = /width/.test(e.message); }
  try { await Parallel.scalarsFromBytes(narrow, n, { width: 8, montgomery: true }); } catch (e) { refusedMont = /Montgomery/.test(e.message); }
  const bad = Buffer.from(montS);
  toBytes(q, 32).copy(bad, 32 * (n - 1));
  try { await Parallel.scalarsFromBytes(bad, n, { montgomery: true }); } catch (e) { range = true; }
  const after = (await Parallel.msm(wide, points, n)).result;
  console.log(JSON.stringify({ plain: show(plain), narrow: show(viaNarrow), mont: show(viaMont), scalarsEqual, pointsEqual, defaults, shortBuffer,
                               refusedWidth, refusedMont, range, after: show(after) }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
