// The argument checks of Parallel.ntt (nttArgs, js/parallel.mjs) over the table of tests/golden/ntt_args_parity.json, which
// tests/golden/make_ntt_fixture.py wrote from the Python twin (ntt_args, msm_zprize_amd/parallel.py).  Host only: no
// context is created and nothing reaches a device.
//   node js/scripts/ntt-args.mjs TABLE.json
//   -> one JSON line: [[label, {ok: checked arguments} | {err: "TypeError" | "ValueError"}], ...]
// Arrays are named in the table (`arrays`: name -> [handle, n, kind]); field elements are {big: decimal}.
import { readFileSync } from "node:fs";
import { nttArgs } from "../parallel.mjs";

const table = JSON.parse(readFileSync(process.argv[2], "utf8"));
const order = BigInt(table.order);
const arr = (v) => (typeof v === "string" && v in table.arrays ? { handle: table.arrays[v][0], n: table.arrays[v][1], kind: table.arrays[v][2] } : v);
const num = (v) => (v !== null && typeof v === "object" ? BigInt(v.big) : v);
const rows = [];
for (const [label, row] of table.cases) {
  const options = {};
  for (const key of ["inverse", "nIn", "count", "first", "firstOut"]) if (key in row) options[key] = row[key];
  for (const key of ["shift", "root"]) if (key in row) options[key] = num(row[key]);
  if ("out" in row) options.out = arr(row.out);
  try {
    const t = nttArgs(arr(row.x), row.logN, options, order);
    for (const key of ["root", "shift"]) t[key] = t[key] === null ? null : t[key].toString();
    rows.push([label, { ok: t }]);
  } catch (e) {
    rows.push([label, { err: e instanceof TypeError ? "TypeError" : "ValueError" }]);
  }
}
console.log(JSON.stringify(rows));
