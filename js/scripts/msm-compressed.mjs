// Compressed point sets from the JavaScript host: pointsFromBytes(bytes, n, {compressed, sign, isInf}) and
// pointsToCompressedBytes(points, {first, count, sign}) (msmz_import_points with MSMZ_SRC_COMPRESSED and
// msmz_download_points_compressed through napi/msmz_napi.c).
//   node js/scripts/msm-compressed.mjs tests/golden/compressed_js_fixture.json
//   -> one JSON line {points, download, range, isInf, msm, noRoot, tooBig, signedZeroRoot, refusedArgs, after}
// points[sign]: the decompressed set reads back as the fixture's points; download[sign]: the compressed download of that
// set, hex, under the OTHER convention as well (four strings); range: records [5, 5 + 20) alone; isInf: the flags of the
// download; msm: an MSM over the decompressed set equals the one over the uploaded points; noRoot / tooBig /
// signedZeroRoot: the status code a planted bad record throws with ("7", "6", "7"); refusedArgs: the host refuses bad
// options before any call; after: the context still decompresses the good records.
import { readFileSync } from "fs";
import { Weierstraß, startThreads, compressedArgs } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const n = fx.n, fb = fx.feBytes;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Affine } = Curve;
  const isInf = Buffer.from(fx.isInf);
  const want = fx.points.map((q) => ({ x: BigInt(q.x), y: BigInt(q.y), isZero: q.isZero }));
  const uploaded = await Affine.fromBigints(want);
  const scalars = Buffer.alloc(32 * n);
  for (let i = 0; i < n; i++) scalars.writeUInt32LE(3 * i + 1, 32 * i);
  const ref = (await Parallel.msm(scalars, uploaded, n)).result;
  const out = { points: {}, download: {}, range: {}, isInf: null, msm: true, refusedArgs: 0 };
  for (const sign of ["largest", "parity"]) {
    const recs = Buffer.from(fx[sign].records, "hex");
    const set = await Parallel.pointsFromBytes(recs, n, { compressed: true, sign, isInf });
    const back = Affine.toBigints(set);
    out.points[sign] = back.length === n && back.every((q, i) => q.isZero === want[i].isZero && (q.isZero || (q.x === want[i].x && q.y === want[i].y)));
    for (const outSign of ["largest", "parity"]) {
      const d = await Parallel.pointsToCompressedBytes(set, { sign: outSign });
      out.download[sign + ">" + outSign] = d.records.toString("hex");
      out.isInf = Array.from(d.isInf);
    }
    out.range[sign] = (await Parallel.pointsToCompressedBytes(set, { first: 5, count: 20, sign })).records.toString("hex");
    const r = (await Parallel.msm(scalars, set, n)).result;
    out.msm = out.msm && r.x === ref.x && r.y === ref.y && r.isZero === ref.isZero;
    set.free();
  }
  const good = Buffer.from(fx.largest.records, "hex");
  for (const key of ["noRoot", "tooBig", "signedZeroRoot"]) {
    const bad = Buffer.from(good);
    Buffer.from(fx[key], "hex").copy(bad, fb * 9);
    try { await Parallel.pointsFromBytes(bad, n, { compressed: true, isInf }); out[key] = "accepted"; } catch (e) { out[key] = e.code; }
  }
  for (const f of [() => compressedArgs("t", 1), () => compressedArgs("t", true, "odd"), () => compressedArgs("t", false, "parity"),
                   () => compressedArgs("t", true, "largest", true), () => Parallel.pointsFromBytes(good, n + 1, { compressed: true }),
                   () => Parallel.pointsToCompressedBytes(scalars), () => Parallel.pointsToCompressedBytes(uploaded, { first: n }),
                   () => Parallel.pointsToCompressedBytes(uploaded, { count: n + 1 }), () => Parallel.pointsToCompressedBytes(uploaded, { sign: "odd" })]) {
    try { await f(); } catch (e) { out.refusedArgs++; }
  }
  const again = await Parallel.pointsFromBytes(good, n, { compressed: true, isInf });
  out.after = Affine.toBigints(again, 0, 3).every((q, i) => q.x === want[i].x && q.y === want[i].y);
  console.log(JSON.stringify(out));
  Curve.close();
}

main().catch((e) => { console.error(e); process.exit(1); });
