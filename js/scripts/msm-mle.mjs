// Multilinear polynomials over resident scalar arrays from the JavaScript host (Parallel.eqTable / evaluateMle / bindMle /
// sumcheckRound over napi scalarsEqTable / scalarsMleEval / scalarsMleBind / scalarsSumcheckRound; msmz_scalars_eq_table /
// _mle_eval / _mle_bind / _sumcheck_round).
//   node js/scripts/msm-mle.mjs FIXTURE.json
//   -> one JSON line {eq, evals, bindHigh, bindLow, inPlace, roundHigh, roundLow, sizes, refused}
// FIXTURE.json (tests/golden/mle_js_fixture.json, written by tests/golden/make_mle_fixture.py) holds three tables of 2^6
// scalars of BLS12-377, a point, a scale, a challenge and two terms of mixed degree, as decimal strings.  eq: the table
// scale eq(point, .); evals: the three tables at the point; bindHigh / bindLow: all three tables (one handle, count 3)
// bound to the challenge; inPlace: table 0 bound in its high variable over its own low half (the whole array is
// returned); roundHigh / roundLow: the round values.  sizes: the addon's descriptor sizes and limits are those the host
// packs by.  refused: a point value >= the group order, a low bind in place, a mask beyond the tables and a range beyond
// the array throw before the device.
import { readFileSync } from "node:fs";
import { createRequire } from "module";
import { Weierstraß, startThreads, SUMCHECK_MAX_TABLES, SUMCHECK_MAX_DEGREE, SUMCHECK_MAX_TERMS } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const v = fx.nVars, n = 2 ** v;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar } = Curve;
  const tables = fx.tables.map((t) => t.map(BigInt));
  const all = await Scalar.fromBigints(tables.flat());            // the three tables in one handle, one after another
  const single = await Promise.all(tables.map((t) => Scalar.fromBigints(t)));
  const point = fx.point.map(BigInt), r = BigInt(fx.r), scale = BigInt(fx.scale);
  const terms = fx.terms.map(([c, mask]) => [c === null ? null : BigInt(c), mask]);
  const show = (arr) => Scalar.toBigints(arr).map((s) => s.toString());
  const eq = show(await Parallel.eqTable(point, scale));
  const evals = [];
  for (let k = 0; k < 3; k++) evals.push((await Parallel.evaluateMle(all, point, { first: k * n })).toString());
  const bindHigh = show(await Parallel.bindMle(all, r, { nVars: v, count: 3 }));
  const bindLow = show(await Parallel.bindMle(all, r, { nVars: v, count: 3, low: true }));
  const same = await Parallel.bindMle(single[0], r, { out: single[0] });
  const inPlace = show(single[0]);
  const spread = [[all, 0], [all, n], [all, 2 * n]];
  const roundHigh = (await Parallel.sumcheckRound(spread, terms, { nVars: v })).map((s) => s.toString());
  const roundLow = (await Parallel.sumcheckRound([all, single[1], [all, 2 * n]], terms, { nVars: v, low: true })).map((s) => s.toString());
  const d = createRequire(import.meta.url)("../msmz_napi.node").descriptorSizes();
  const sizes = d.mleBind === 40 && d.sumcheck === 32 && d.sumcheckTable === 16 && d.sumcheckTerm === 16 &&
    d.maxTables === SUMCHECK_MAX_TABLES && d.maxDegree === SUMCHECK_MAX_DEGREE && d.maxTerms === SUMCHECK_MAX_TERMS;
  let refused = 0;
  for (const bad of [() => Parallel.eqTable([curveParams.order]), () => Parallel.bindMle(single[1], r, { low: true, out: single[1] }),
                     () => Parallel.sumcheckRound([all], [[null, 2]], { nVars: v }), () => Parallel.evaluateMle(all, point, { first: 2 * n + 1 })]) {
    try {
      await bad();
    } catch (e) {
      if (/eqTable|bindMle|sumcheckRound|evaluateMle/.test(e.message)) refused++;
    }
  }
  Curve.close();
  console.log(JSON.stringify({ eq, evals, bindHigh, bindLow, inPlace, roundHigh, roundLow, sizes, refused: refused === 4 && same === single[0] }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
