// Batched MSM from the JavaScript host: B vectors against one resident point set (Parallel.msmBatch).
//   node js/scripts/msm-batch.mjs LOG2N B [--glv G]  -> one JSON line {resident: [...], host: [...], refused: bool}
// Points: randomPointsFast(2^LOG2N, seed 1).  resident: randomScalars(B * 2^LOG2N, seed 2) as ONE array.  host: vector
// k holds the scalars k * 1000 + i + 1 (32-byte little-endian).  refused: a list of resident arrays throws.
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const args = process.argv.slice(2);
  const n = 1 << Number(args[0] || 10);
  const B = Number(args[1] || 3);
  const glv = args.includes("--glv") ? Number(args[args.indexOf("--glv") + 1]) : -1;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel } = Curve;
  const [points] = await Parallel.randomPointsFast(n, { seed: 1n });
  const [scalars] = await Parallel.randomScalars(B * n, { seed: 2n });
  const show = (ps) => ps.map((p) => ({ x: p.x.toString(), y: p.y.toString(), isZero: p.isZero }));
  const resident = await Parallel.msmBatchUnsafe(scalars, points, n, { glv });
  const host = [];
  for (let k = 0; k < B; k++) {
    const v = Buffer.alloc(32 * n);
    for (let i = 0; i < n; i++) v.writeUInt32LE(k * 1000 + i + 1, 32 * i);
    host.push(v);
  }
  const hostRes = await Parallel.msmBatch(host, points, n, { glv });
  let refused = false;
  try {
    await Parallel.msmBatch([scalars, scalars], points, n);
  } catch (e) {
    refused = /not accepted/.test(e.message);
  }
  console.log(JSON.stringify({ resident: show(resident), host: show(hostRes), refused }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
