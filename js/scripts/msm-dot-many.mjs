// The batched inner products from the JavaScript host (Parallel.innerProducts / evaluatePolynomials over napi
// scalarsDotMany; msmz_scalars_dot_many).
//   node js/scripts/msm-dot-many.mjs FIXTURE.json
//   -> one JSON line {values, resident, around, pairs, evals, sizes, refused}
// FIXTURE.json (tests/golden/dot_many_js_fixture.json, written by tests/golden/make_dot_many_fixture.py) holds 6 rows and
// 3 columns of 70 scalars of BLS12-377 and two points, as decimal strings.  values: the 6 x 3 inner products to the
// host; resident: the same through entries [2, 20) of an array of 23, around: that array's other five entries
// (untouched); pairs: innerProduct pair by pair equals them; evals: the rows as polynomials at the two points
// (evaluatePolynomials).  sizes: the addon's descriptor sizes and limits are those the host packs by.  refused: too many
// columns, an n beyond a vector, a destination on an input and a point >= the group order throw before the device.
import { readFileSync } from "node:fs";
import { createRequire } from "module";
import { Weierstraß, startThreads, DOT_MANY_MAX_ROWS, DOT_MANY_MAX_COLS } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar } = Curve;
  const str = (m) => m.map((r) => r.map((v) => v.toString()));
  const rows = [], cols = [];
  for (const r of fx.rows) rows.push(await Scalar.fromBigints(r.map(BigInt)));
  for (const c of fx.cols) cols.push(await Scalar.fromBigints(c.map(BigInt)));
  const values = await Parallel.innerProducts(rows, cols, fx.n);
  const results = rows.length * cols.length;
  const dest = await Scalar.fromBigints(Array.from({ length: results + 5 }, () => 7n));
  if ((await Parallel.innerProducts(rows, cols, null, { out: dest, firstOut: 2 })) !== dest) throw Error("out");
  const all = await Scalar.toBigints(dest);
  const resident = Array.from({ length: rows.length }, (_, r) => all.slice(2 + r * cols.length, 2 + (r + 1) * cols.length).map((v) => v.toString()));
  const around = [...all.slice(0, 2), ...all.slice(2 + results)].map((v) => v.toString());
  let pairs = true;
  for (let r = 0; r < rows.length; r++)
    for (let c = 0; c < cols.length; c++) pairs = pairs && (await Parallel.innerProduct(rows[r], cols[c], fx.n)) === values[r][c];
  const evals = await Parallel.evaluatePolynomials(rows, fx.points.map(BigInt), fx.n);
  const addon = createRequire(import.meta.url)("../msmz_napi.node");
  const d = addon.descriptorSizes("dotMany");
  const sizes = d.dotMany === 48 && d.scalarVec === 16 && d.maxRows === DOT_MANY_MAX_ROWS && d.maxCols === DOT_MANY_MAX_COLS &&
    addon.descriptorSizes().dotMany === undefined;
  let refused = 0;
  for (const bad of [() => Parallel.innerProducts(rows, Array(9).fill(cols[0])), () => Parallel.innerProducts(rows, cols, fx.n + 1),
                     () => Parallel.innerProducts([[dest, 0]], [[dest, 10]], 8, { out: dest, firstOut: 7 }),
                     () => Parallel.evaluatePolynomials(rows, [curveParams.order])]) {
    try {
      await bad();
    } catch (e) {
      if (/innerProducts|evaluatePolynomials/.test(e.message)) refused++;
    }
  }
  Curve.close();
  console.log(JSON.stringify({ values: str(values), resident, around, pairs, evals: str(evals), sizes, refused: refused === 4 }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
