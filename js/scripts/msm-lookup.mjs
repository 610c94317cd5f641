// The multiplicities of a column in a table from the JavaScript host (Parallel.lookupMultiplicities over napi
// scalarsLookup; msmz_scalars_lookup).
//   node js/scripts/msm-lookup.mjs FIXTURE.json
//   -> one JSON line {multiplicities, positions, info, plain, intoRange, sizes, refused}
// FIXTURE.json (tests/golden/lookup_js_fixture.json, written by tests/golden/make_lookup_fixture.py) holds a table of 48
// BLS12-377 scalars with duplicates and a column of 200 with entries that are in no table, scalars as decimal strings.
// multiplicities / positions / info: one call with positions; plain: the result words of a call without them (no
// positions key); intoRange: the multiplicities written behind table and column in one array of 48 + 200 + 48 entries
// (the whole array is returned); sizes: the addon's descriptor sizes are those of the header; refused: a destination
// that meets the table, one that meets the column, a column range beyond its array and a point array throw before the
// device.
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
  const table = fx.table.map(BigInt), column = fx.column.map(BigInt);
  const show = (arr) => Scalar.toBigints(arr).map((s) => s.toString());
  const ta = await Scalar.fromBigints(table), fa = await Scalar.fromBigints(column);
  const [m, info] = await Parallel.lookupMultiplicities(fa, ta, { positions: true });
  const positions = Array.from(info.positions);
  delete info.positions;
  const [m2, plain] = await Parallel.lookupMultiplicities(fa, ta);
  const same = show(m2).join() === show(m).join();
  const T = table.length, F = column.length;
  const all = await Scalar.fromBigints(table.concat(column, table));
  const [into] = await Parallel.lookupMultiplicities(all, all, { firstColumn: T, n: F, tableN: T, out: all, firstOut: T + F });
  const d = N.descriptorSizes("lookup");
  const sizes = d.lookup === 64 && d.lookupResult === 24 && d.none === 0xffffffff && N.descriptorSizes().lookup === undefined;
  let refused = 0;
  for (const bad of [() => Parallel.lookupMultiplicities(all, all, { firstColumn: T, n: F, tableN: T, out: all, firstOut: T - 1 }),
                     () => Parallel.lookupMultiplicities(all, all, { firstColumn: T, n: F, tableN: T, out: all, firstOut: T + F - 1 }),
                     () => Parallel.lookupMultiplicities(fa, ta, { firstColumn: 1, n: F }),
                     () => Parallel.lookupMultiplicities(fa, { handle: 1, n: 4, kind: "points" })]) {
    try {
      await bad();
    } catch (e) {
      if (/lookupMultiplicities/.test(e.message)) refused++;
    }
  }
  const out = { multiplicities: show(m), positions, info, plain, intoRange: show(all), sizes, refused: refused === 4 && same && into === all };
  Curve.close();
  console.log(JSON.stringify(out));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
