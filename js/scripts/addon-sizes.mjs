// The N-API addon sizes every Buffer a point goes into from the library (msmz_ctx_fe_bytes / msmz_curve_fe_bytes), not
// from the feBytes argument: a value that disagrees is refused with code "1" before anything is allocated or called.
//   node js/scripts/addon-sizes.mjs --cpu   -> {pointAdd: [[label, code | null, isInf | null], ...]}      (no device)
//   node js/scripts/addon-sizes.mjs         -> {refused: {call: code}, same: {call: bool}}                (one GPU)
// refused: downloadPoints, msm, msmBatch and msmSegments of the addon with feBytes = 8 on a BLS12-377 context (48) of 8
// points and 8 scalars; same: the calls with 48 give what Parallel gives.
import { createRequire } from "module";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

const addon = createRequire(import.meta.url)("../msmz_napi.node");
const attempt = (fn) => {
  try {
    return [null, fn()];
  } catch (e) {
    return [e.code === undefined ? "none" : e.code, null];
  }
};

function cpu() {
  const rows = [];
  const add = (label, ...args) => {
    const [code, r] = attempt(() => addon.pointAdd(...args));
    rows.push([label, code, r === null ? null : r.isInf]);
  };
  add("feBytes 8 for a 48-byte curve", 0, Buffer.alloc(96), Buffer.alloc(96), 8);
  add("a 4-byte input", 0, Buffer.alloc(4), Buffer.alloc(96), 48);
  add("a 95-byte second input", 0, null, Buffer.alloc(95), 48);
  add("curve 9", 9, Buffer.alloc(96), Buffer.alloc(96), 48);
  add("curve 9, feBytes 0", 9, null, null, 0);
  add("feBytes 32 for a 48-byte curve", 0, null, null, 32);
  add("a short argument list", 0, null, null);
  add("zero + zero", 0, null, null, 48);
  add("zero + zero, 32-byte curve", 1, null, null, 32);
  console.log(JSON.stringify({ pointAdd: rows }));
}

async function gpu() {
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Affine } = Curve;
  const ctx = Curve._ctx, n = 8;
  const points = await Parallel.randomPointsFast(n), scalars = await Parallel.randomScalars(n);
  const table = Buffer.alloc(24);
  table.writeBigUInt64LE(BigInt(n), 16);   // one segment: [0, 0, n]
  const calls = {
    downloadPoints: (fb) => addon.downloadPoints(ctx, points.handle, 0, 1, fb),
    msm: (fb) => addon.msm(ctx, points.handle, scalars.handle, n, fb, {}).xy,
    msmBatch: (fb) => addon.msmBatch(ctx, points.handle, scalars.handle, n, 1, fb, {}).xy,
    msmSegments: (fb) => addon.msmSegments(ctx, points.handle, scalars.handle, table, 1, fb, {}).xy,
  };
  const hex = (p) => [p.x, p.y].map((v) => v.toString(16).padStart(96, "0"));
  const leHex = (buf) => [0, 48].map((o) => Buffer.from(buf.subarray(o, o + 48)).reverse().toString("hex"));
  const msm = (await Parallel.msm(scalars, points, n)).result;
  const want = { downloadPoints: Affine.toBigints(points, 0, 1)[0], msm, msmBatch: (await Parallel.msmBatch(scalars, points, n))[0],
                 msmSegments: (await Parallel.msmSegments(scalars, points, [[0, 0, n]]))[0] };
  const refused = {}, same = {};
  for (const [name, call] of Object.entries(calls)) {
    refused[name] = attempt(() => call(8))[0];
    const [code, xy] = attempt(() => call(48));
    same[name] = code === null && xy.length === 96 && !want[name].isZero && JSON.stringify(leHex(xy)) === JSON.stringify(hex(want[name]));
  }
  Curve.close();
  console.log(JSON.stringify({ refused, same }));
}

(process.argv.includes("--cpu") ? Promise.resolve(cpu()) : gpu()).catch((e) => {
  console.error(e);
  process.exit(1);
});
