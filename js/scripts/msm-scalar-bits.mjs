// The scalar bit bound from the JavaScript host (options.scalarBits).
//   node js/scripts/msm-scalar-bits.mjs LOG2N B BITS
//   -> one JSON line {bounded, plain, K, Kplain, batch, pre, info, refused, range, after}
// Points: randomPointsFast(2^LOG2N, seed 1); host scalars: vector k, entry i = i + 1000 k + 1 (far below 2^BITS).
// bounded / plain: msmUnsafe of vector 0 with and without the bound (K / Kplain: the windows each ran); batch: msmBatch of
// the B vectors with the bound; pre: msm of vector 0 over a set precomputed for the bound (info: its parameters);
// refused: scalarBits 300 throws before the device; range: a scalar equal to 2^BITS under the bound throws; after: the
// same context then computes vector 0 again.
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const args = process.argv.slice(2);
  const n = 1 << Number(args[0] || 10);
  const B = Number(args[1] || 3);
  const bits = Number(args[2] || 64);
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel } = Curve;
  const [points] = await Parallel.randomPointsFast(n, { seed: 1n });
  const vector = (k) => {
    const b = Buffer.alloc(32 * n);
    for (let i = 0; i < n; i++) b.writeUInt32LE(i + 1000 * k + 1, 32 * i);
    return b;
  };
  const vecs = [];
  for (let k = 0; k < B; k++) vecs.push(vector(k));
  const show = (p) => ({ x: p.x.toString(), y: p.y.toString(), isZero: p.isZero });
  const opt = { scalarBits: bits, glv: 0 };
  const r1 = await Parallel.msmUnsafe(vecs[0], points, n, false, opt);
  const r0 = await Parallel.msmUnsafe(vecs[0], points, n, false, { glv: 0 });
  const batch = await Parallel.msmBatch(vecs, points, n, opt);
  const pre = await Parallel.precomputePoints(points, n, opt, 0);
  const viaPre = (await Parallel.msm(vecs[0], pre, n)).result;
  let refused = false, range = false;
  try {
    await Parallel.msm(vecs[0], points, n, false, { scalarBits: 300 });
  } catch (e) {
    refused = /scalarBits/.test(e.message);
  }
  const bad = Buffer.from(vecs[0]);
  bad.fill(0, 32 * (n - 1), 32 * n);
  bad[32 * (n - 1) + (bits >> 3)] = 1 << (bits & 7);   // = 2^bits
  try {
    await Parallel.msm(bad, points, n, false, opt);
  } catch (e) {
    range = true;
  }
  const after = (await Parallel.msm(vecs[0], points, n, false, opt)).result;
  pre.free();
  console.log(JSON.stringify({ bounded: show(r1.result), plain: show(r0.result), K: r1.stats.K, Kplain: r0.stats.K,
                               batch: batch.map(show), pre: show(viaPre), info: pre.info, refused, range, after: show(after) }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
