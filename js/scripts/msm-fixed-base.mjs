// Fixed-base multiplication from the JavaScript host (Parallel.fixedBaseMul over napi fixedBaseMul,
// msmz_points_fixed_base).
//   node js/scripts/msm-fixed-base.mjs FIXTURE.json
//   -> one JSON line {generator, affine, resident, bounded64, srs, same, refused, range}
// FIXTURE.json (tests/golden/fixed_base_js_fixture.json, written by tests/golden/make_fixed_base_fixture.py) holds n
// BLS12-377 scalars, n scalars below 2^64, a base B = [k]G, tau, and what the oracle says the calls owe -- all as
// decimal strings.  generator: [s_i]G (base null); affine: [s_i]B from the affine point; resident: the same from a
// resident point array at baseIndex 1, over the second half of the scalars (firstScalar = n / 2); bounded64: [t_i]B
// with scalarBits = 64; srs: [tau^i]G from scalarPowers(tau, n) -- each as [{x, y, isZero}, ...].  same: mulPoints over n
// copies of B gives the points of `affine`.  refused: a point array as scalars, a bad base, a baseIndex beyond the
// array and a bad scalarBits throw before the device; range: scalars beyond their bound fail the call and the next
// call works.
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
  const B = point(fx.base);
  const scalars = await Scalar.fromBigints(fx.scalars.map(BigInt));
  const scalars64 = await Scalar.fromBigints(fx.scalars64.map(BigInt));
  const show = (arr) => Affine.toBigints(arr).map((p) => ({ x: p.x.toString(), y: p.y.toString(), isZero: !!p.isZero }));
  const half = n >> 1;
  const holder = await Affine.fromBigints([point(fx.other), B]);
  const generator = show(await Parallel.fixedBaseMul(scalars, n));
  const affine = show(await Parallel.fixedBaseMul(scalars, n, { base: B }));
  const resident = show(await Parallel.fixedBaseMul(scalars, n - half, { base: holder, baseIndex: 1, firstScalar: half }));
  const bounded64 = show(await Parallel.fixedBaseMul(scalars64, n, { base: B, scalarBits: 64 }));
  const srs = show(await Parallel.fixedBaseMul(await Parallel.scalarPowers(BigInt(fx.tau), n)));
  const copies = await Affine.fromBigints(Array(n).fill(B));
  const same = JSON.stringify(show(await Parallel.mulPoints(scalars, copies, n))) === JSON.stringify(affine);
  let refused = 0;
  for (const bad of [() => Parallel.fixedBaseMul(holder, 2), () => Parallel.fixedBaseMul(scalars, n, { base: 5n }),
                     () => Parallel.fixedBaseMul(scalars, n, { base: holder, baseIndex: 2 }),
                     () => Parallel.fixedBaseMul(scalars, n, { baseIndex: 1 }),
                     () => Parallel.fixedBaseMul(scalars, n, { scalarBits: 257 }),
                     () => Parallel.fixedBaseMul(scalars, n + 1)]) {
    try {
      await bad();
    } catch (e) {
      if (/fixedBaseMul/.test(e.message)) refused++;
    }
  }
  let range = false;
  try {
    await Parallel.fixedBaseMul(scalars, n, { base: B, scalarBits: 64 });
  } catch (e) {
    range = /msmz_points_fixed_base/.test(e.message);
  }
  range = range && JSON.stringify(show(await Parallel.fixedBaseMul(scalars64, n, { base: B, scalarBits: 64 }))) === JSON.stringify(bounded64);
  console.log(JSON.stringify({ generator, affine, resident, bounded64, srs, same, refused: refused === 6, range }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
