// Precomputed point set from the JavaScript host (Parallel.precomputePoints).
//   node js/scripts/msm-precompute.mjs LOG2N B [--glv G] [--factor F]
//   -> one JSON line {info, plain, single, batch, batchPlain, refused}
// Points: randomPointsFast(2^LOG2N, seed 1); scalars: randomScalars(B * 2^LOG2N, seed 2) as ONE array.  single: msm of
// vector 0 over the precomputed set; batch / batchPlain: msmBatchUnsafe of all B vectors over the precomputed / plain
// set; plain: msm of vector 0 over the plain set.  refused: factor 1 throws.
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const args = process.argv.slice(2);
  const n = 1 << Number(args[0] || 10);
  const B = Number(args[1] || 3);
  const opt = (name, dflt) => (args.includes(name) ? Number(args[args.indexOf(name) + 1]) : dflt);
  const glv = opt("--glv", -1);
  const factor = opt("--factor", 0);
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel } = Curve;
  const [points] = await Parallel.randomPointsFast(n, { seed: 1n });
  const [scalars] = await Parallel.randomScalars(B * n, { seed: 2n });
  const [first] = await Parallel.randomScalars(n, { seed: 2n });
  const show = (p) => ({ x: p.x.toString(), y: p.y.toString(), isZero: p.isZero });
  const pre = await Parallel.precomputePoints(points, n, { glv }, factor);
  const plain = (await Parallel.msmUnsafe(first, points, n)).result;
  const single = (await Parallel.msm(first, pre, n)).result;
  const batch = await Parallel.msmBatchUnsafe(scalars, pre, n);
  const batchPlain = await Parallel.msmBatchUnsafe(scalars, points, n);
  let refused = false;
  try {
    await Parallel.precomputePoints(points, n, {}, 1);
  } catch (e) {
    refused = /factor/.test(e.message);
  }
  pre.free();
  console.log(JSON.stringify({ info: pre.info, plain: show(plain), single: show(single), batch: batch.map(show),
                               batchPlain: batchPlain.map(show), refused }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
