// The sumcheck step from the JavaScript host (Parallel.sumcheckStep / sumcheckProve over napi scalarsSumcheckStep;
// msmz_scalars_sumcheck_step).
//   node js/scripts/msm-sumcheck-step.mjs FIXTURE.json
//   -> one JSON line {high, low, sizes, refused}, high and low each {steps, tables, last, lastTables, polys, claim}
// FIXTURE.json (tests/golden/sumcheck_step_js_fixture.json, written by tests/golden/make_sumcheck_step_fixture.py) holds
// three tables of 2^6 scalars of BLS12-377, two terms of mixed degree and six challenges, as decimal strings.  Per order:
// steps: the values of three consecutive steps over the first three challenges (high: every table in place; low: into
// other arrays, there and back); tables: the three tables of 2^3 entries they leave; last, lastTables: the last-variable
// step (nVars 1) on entries [0, 2) of those tables with the fourth challenge, its value and the bound entries; polys,
// claim: sumcheckProve over all six challenges on fresh copies.  sizes: the addon's descriptor sizes are those the host
// packs by.  refused: a challenge >= the group order, the low order in place, the high half as a destination, a
// destination on another table and a missing destination throw before the device.
import { readFileSync } from "node:fs";
import { createRequire } from "module";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const v = fx.nVars, n = 2 ** v;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar } = Curve;
  const data = fx.tables.map((t) => t.map(BigInt));
  const rs = fx.challenges.map(BigInt);
  const terms = fx.terms.map(([c, mask]) => [c === null ? null : BigInt(c), mask]);
  const str = (xs) => xs.map((s) => s.toString());
  const show = async (arr, first, count) => str((await Scalar.toBigints(arr)).slice(first, first + count));
  const result = {};
  for (const low of [false, true]) {
    let cur = await Promise.all(data.map((t) => Scalar.fromBigints(t)));
    let other = low ? await Promise.all(data.map((t) => Scalar.fromBigints(t.slice(0, n / 2)))) : null;
    const steps = [];
    for (let k = 0; k < 3; k++) {
      const { degree, values } = await Parallel.sumcheckStep(cur, terms, rs[k], { nVars: v - k, out: other, low });
      if (degree !== values.length - 1) throw Error("degree");
      steps.push(str(values));
      if (low) [cur, other] = [other, cur];
    }
    const tables = [];
    for (const t of cur) tables.push(await show(t, 0, 2 ** (v - 3)));
    const last = await Parallel.sumcheckStep(cur, terms, rs[3], { nVars: 1, out: low ? other : null, low });
    if (last.degree !== 0 || last.values.length !== 1) throw Error("last");
    const lastTables = [];
    for (const t of low ? other : cur) lastTables.push((await show(t, 0, 1))[0]);
    const fresh = await Promise.all(data.map((t) => Scalar.fromBigints(t)));
    let at = 0;
    const proof = await Parallel.sumcheckProve(fresh, terms, v, async () => rs[at++], { low });
    if (proof.challenges.length !== v || proof.challenges.some((r, k) => r !== rs[k])) throw Error("challenges");
    result[low ? "low" : "high"] = { steps, tables, last: last.values[0].toString(), lastTables, polys: proof.polys.map(str),
      claim: proof.claim.toString() };
  }
  const f = await Scalar.fromBigints(data[0]), g = await Scalar.fromBigints(data[1]);
  const d = createRequire(import.meta.url)("../msmz_napi.node").descriptorSizes("sumcheckStep");
  const sizes = d.sumcheckStep === 48 && d.sumcheckTable === 16 && d.sumcheckTerm === 16 &&
    createRequire(import.meta.url)("../msmz_napi.node").descriptorSizes().sumcheckStep === undefined;
  let refused = 0;
  const one = [[null, 1]];
  for (const bad of [() => Parallel.sumcheckStep([f], one, curveParams.order), () => Parallel.sumcheckStep([f], one, 5n, { low: true }),
                     () => Parallel.sumcheckStep([f], one, 5n, { out: [[f, n / 2]] }), () => Parallel.sumcheckStep([f, g], [[null, 3]], 5n, { out: [g, f] }),
                     () => Parallel.sumcheckStep([f, g], [[null, 3]], 5n, { out: [g] })]) {
    try {
      await bad();
    } catch (e) {
      if (/sumcheckStep/.test(e.message)) refused++;
    }
  }
  Curve.close();
  console.log(JSON.stringify({ ...result, sizes, refused: refused === 5 }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
