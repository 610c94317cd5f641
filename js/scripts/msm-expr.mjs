// Gate expressions from the JavaScript host (Parallel.evaluateExpression over napi scalarsExpr; msmz_scalars_expr).
//   node js/scripts/msm-expr.mjs FIXTURE.json
//   -> one JSON line {values: {name: [...]}, accumulated, intoRange, sizes, refused}
// FIXTURE.json (tests/golden/expr_js_fixture.json, written by tests/golden/make_expr_fixture.py) holds eight columns of
// 70 BLS12-377 scalars and five expressions with their expected values, scalars as decimal strings.  values: every
// expression into a new array; accumulated: out = y out + gate over the first three expressions, each call in place
// with the term [y, [out]] next to the gate's; intoRange: the first expression written behind two columns in one array
// of 3 n entries (the whole array is returned); sizes: the addon's descriptor sizes and limits are those of the header;
// refused: a destination that overlaps an unrotated column in part, one that is a rotated column's own range, a column
// index out of range, a coefficient that is not below the group order and a point array throw before the device.
import { readFileSync } from "node:fs";
import { createRequire } from "module";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar } = Curve;
  const N = createRequire(import.meta.url)("../msmz_napi.node");
  const n = fx.n;
  const show = (arr) => Scalar.toBigints(arr).map((s) => s.toString());
  const terms = (name) => fx.expressions[name].terms.map(([c, fs]) => [c === null ? null : BigInt(c), fs]);
  const cols = [];
  for (const col of fx.columns) cols.push(await Scalar.fromBigints(col.map(BigInt)));
  const values = {};
  for (const name of Object.keys(fx.expressions)) {
    const out = await Parallel.evaluateExpression(cols, terms(name));
    values[name] = show(out);
    out.free();
  }
  const y = BigInt(fx.y);
  const acc = await Scalar.fromBigints(Array(n).fill(0n));
  let same = true;
  for (const name of ["plonk", "permutation", "sbox"])
    same = (await Parallel.evaluateExpression(cols.concat([acc]), terms(name).concat([[y, [cols.length]]]), { out: acc })) === acc && same;
  const all = await Scalar.fromBigints(fx.columns[5].concat(fx.columns[6], fx.columns[5]).map(BigInt));
  const shifted = cols.map((c, k) => (k === 5 ? [all, 0] : k === 6 ? [all, n] : c));
  same = (await Parallel.evaluateExpression(shifted, terms("plonk"), { n, out: all, firstOut: 2 * n })) === all && same;
  const d = N.descriptorSizes("expr");
  const sizes = d.exprColumn === 16 && d.exprFactor === 8 && d.exprTerm === 24 && d.expr === 40 && d.maxColumns === 16 &&
    d.maxTerms === 32 && d.maxDegree === 8 && d.maxOperands === 32 && N.descriptorSizes().expr === undefined;
  let refused = 0;
  for (const bad of [() => Parallel.evaluateExpression([[all, 0]], [[null, [0]]], { n, out: all, firstOut: 1 }),
                     () => Parallel.evaluateExpression([[all, 0]], [[null, [[0, 1]]]], { n, out: all }),
                     () => Parallel.evaluateExpression([cols[0]], [[null, [1]]]),
                     () => Parallel.evaluateExpression([cols[0]], [[curveParams.order, [0]]]),
                     () => Parallel.evaluateExpression([{ handle: 1, n: 4, kind: "points" }], [[null, [0]]])]) {
    try {
      await bad();
    } catch (e) {
      if (/evaluateExpression/.test(e.message)) refused++;
    }
  }
  const out = { values, accumulated: show(acc), intoRange: show(all), sizes, refused: refused === 5 && same };
  Curve.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
