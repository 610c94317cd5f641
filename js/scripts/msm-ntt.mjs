// Number-theoretic transforms over resident scalar arrays from the JavaScript host (Parallel.ntt / rootOfUnity over napi
// scalarsNtt / scalarsRootOfUnity; msmz_scalars_ntt / _root_of_unity).
//   node js/scripts/msm-ntt.mjs FIXTURE.json
//   -> one JSON line {roots, forward, coset, cosetInverse, short, mirrored, roundTrip, inPlace, product, refused}
// FIXTURE.json (tests/golden/ntt_js_fixture.json, written by tests/golden/make_ntt_fixture.py) holds 2^small scalars x of
// BLS12-377 as decimal strings and a coset shift; X_i = x[i mod 2^small] (i + 1) is the long vector of 2^logN entries.
// roots: the default roots at rootLogs; forward: the transform of X (a two-pass plan) at the indices `samples`;
// coset / cosetInverse: the forward and the inverse transform of x on the coset;
// short: two transforms of 2^small entries from inputs of 16 entries each, in one call; mirrored: the transform with the
// inverse of the default root -- scalars as decimal strings.  roundTrip: inverse(forward(x)) is x, on the coset too;
// inPlace: the forward transform written over a copy of X equals the one into a new array; product: a polynomial product through
// ntt, combineScalars and the inverse ntt equals the schoolbook product; refused: a shift of 0n, an inverse with a short
// input, a partly overlapping destination and a root that is not one throw.
import { readFileSync } from "node:fs";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const logN = fx.logN, small = fx.small, n = 2 ** logN, m = 2 ** small, q = curveParams.order;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar } = Curve;
  const xs = fx.x.map(BigInt), shift = BigInt(fx.shift);
  const x = await Scalar.fromBigints(xs);
  const long = Array.from({ length: n }, (_, i) => (xs[i % m] * BigInt(i + 1)) % q);
  const X = await Scalar.fromBigints(long);
  const text = (arr, first, count) => Scalar.toBigints(arr, first, count).map((s) => s.toString());
  const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);
  const roots = fx.rootLogs.map((k) => Parallel.rootOfUnity(k).toString());
  const y = await Parallel.ntt(X, logN);
  const whole = text(y);
  const forward = fx.samples.map((k) => whole[k]);
  const back = await Parallel.ntt(y, logN, { inverse: true });
  const c = await Parallel.ntt(x, small, { shift });
  const coset = text(c);
  const cosetBack = await Parallel.ntt(c, small, { inverse: true, shift });
  const cosetInverse = text(await Parallel.ntt(x, small, { inverse: true, shift }));
  const short = text(await Parallel.ntt(x, small, { nIn: 16, count: 2 }));
  const ws = Parallel.rootOfUnity(small);
  let winv = 1n;
  for (let i = 0; i < m - 1; i++) winv = (winv * ws) % q;   // ws^(m - 1) = ws^-1
  const mirrored = text(await Parallel.ntt(x, small, { root: winv }));
  const roundTrip = same(text(back), long.map(String)) && same(text(cosetBack), fx.x);
  const copy = await Parallel.combineScalars(1n, X);
  const inPlace = (await Parallel.ntt(copy, logN, { out: copy })) === copy && same(text(copy), whole);
  // (a_0 + .. + a_31 X^31) (b_0 + .. + b_31 X^31): a = x[0, 32), b = x[32, 64), transforms of length 64
  const ev = await Parallel.ntt(x, small, { nIn: 32, count: 2 });
  const pointwise = await Parallel.combineScalars(ev, ev, null, null, m, { firstX: m });
  const prod = Scalar.toBigints(await Parallel.ntt(pointwise, small, { inverse: true }));
  const want = Array(m).fill(0n);
  for (let i = 0; i < 32; i++) for (let j = 0; j < 32; j++) want[i + j] = (want[i + j] + xs[i] * xs[32 + j]) % q;
  const product = prod.every((v, i) => v === want[i]);
  let refused = 0;
  for (const bad of [() => Parallel.ntt(x, small, { shift: 0n }), () => Parallel.ntt(x, small, { inverse: true, nIn: 8 }),
                     () => Parallel.ntt(copy, small, { out: copy, firstOut: 1 }), () => Parallel.ntt(x, small, { root: 5n })]) {
    try {
      await bad();
    } catch (e) {
      if (/ntt/.test(e.message)) refused++;
    }
  }
  console.log(JSON.stringify({ roots, forward, coset, cosetInverse, short, mirrored, roundTrip, inPlace, product, refused: refused === 4 }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
