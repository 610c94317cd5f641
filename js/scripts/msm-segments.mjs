// Segmented MSM from the JavaScript host (Parallel.msmSegments over napi msmSegments, msmz_msm_segments).
//   node js/scripts/msm-segments.mjs FIXTURE.json  -> one JSON line {safe, unsafe, ipa, refused}
// FIXTURE.json (tests/golden/segments_js_fixture.json, written by tests/golden/make_segments_fixture.py) holds n points
// and m scalars of BLS12-377 as decimal strings and a list of segments [firstPoint, firstScalar, n].  safe / unsafe: the
// results of msmSegments / msmSegmentsUnsafe, one {x, y, isZero} per segment, in the fixture's order; ipa: the L and R of
// an IPA round over the halves of the point set, [[n/2, 0, n/2], [0, n/2, n/2]]; refused: an empty list, a range beyond
// the set and host scalars throw before the device.
import { readFileSync } from "node:fs";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Affine, Scalar } = Curve;
  const points = await Affine.fromBigints(fx.points.map((p) => ({ x: BigInt(p.x), y: BigInt(p.y), isZero: !!p.isZero })));
  const scalars = await Scalar.fromBigints(fx.scalars.map(BigInt));
  const show = (ps) => ps.map((p) => ({ x: p.x.toString(), y: p.y.toString(), isZero: !!p.isZero }));
  const safe = await Parallel.msmSegments(scalars, points, fx.segments);
  const unsafe = await Parallel.msmSegmentsUnsafe(scalars, points, fx.segments, { glv: 1 });
  const h = fx.points.length >> 1;
  const ipa = await Parallel.msmSegments(scalars, points, [[h, 0, h], [0, h, h]]);
  let refused = 0;
  for (const bad of [() => Parallel.msmSegments(scalars, points, []), () => Parallel.msmSegments(scalars, points, [[1, 0, fx.points.length]]),
                     () => Parallel.msmSegments(Buffer.alloc(32), points, [[0, 0, 1]])]) {
    try {
      await bad();
    } catch (e) {
      if (/msmSegments/.test(e.message)) refused++;
    }
  }
  console.log(JSON.stringify({ safe: show(safe), unsafe: show(unsafe), ipa: show(ipa), refused: refused === 3 }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
