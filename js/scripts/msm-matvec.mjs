// Sparse matrices against resident scalar arrays from the JavaScript host (Parallel.sparseMatrix / matVec over napi
// matrixCreate / matrixInfo / matrixMul; msmz_matrix_create / _matrix_info / _matrix_mul).
//   node js/scripts/msm-matvec.mjs FIXTURE.json
//   -> one JSON line {mx, mty, mxOnes, mtyOnes, intoRange, info, sizes, refused}
// FIXTURE.json (tests/golden/matvec_js_fixture.json, written by tests/golden/make_matvec_fixture.py) holds the triples of
// a 40 x 48 matrix of BLS12-377 scalars in shuffled order and a vector for each orientation, scalars as decimal strings.
// mx / mty: the plain and the transposed product of ONE matrix built for both, its values from a resident array;
// mxOnes / mtyOnes: the same without values (two matrices, one per orientation, a Uint32Array and a bigint-free call);
// intoRange: M x written behind x in one array of nCols + nRows entries (the whole array is returned); info: what
// matrixInfo reports; sizes: the addon's descriptor sizes and flags are those the host packs by.  refused: an index out of
// range, the transposed product of a rows-only matrix, a destination that meets x and a value >= the group order throw
// before the device.
import { readFileSync } from "node:fs";
import { createRequire } from "module";
import { Weierstraß, startThreads } from "../parallel.mjs";
import { bls12377Params as curveParams } from "../concrete/params.mjs";

async function main() {
  const fx = JSON.parse(readFileSync(process.argv[2], "utf8"));
  const [nRows, nCols] = fx.shape;
  await startThreads();
  const Curve = await Weierstraß.create(curveParams);
  const { Parallel, Scalar } = Curve;
  const N = createRequire(import.meta.url)("../msmz_napi.node");
  const values = fx.values.map(BigInt), x = fx.x.map(BigInt), y = fx.y.map(BigInt);
  const show = (arr) => Scalar.toBigints(arr).map((s) => s.toString());
  const xa = await Scalar.fromBigints(x), ya = await Scalar.fromBigints(y), va = await Scalar.fromBigints(values);
  const m = await Parallel.sparseMatrix(fx.rows, fx.cols, va, { shape: fx.shape, orientations: "both" });
  va.free();                                                   // the matrix keeps its own copy
  const mx = show(await Parallel.matVec(m, xa));
  const mty = show(await Parallel.matVec(m, ya, { transpose: true }));
  const rowsOnly = await Parallel.sparseMatrix(Uint32Array.from(fx.rows), fx.cols, null, { shape: fx.shape });
  const colsOnly = await Parallel.sparseMatrix(fx.rows, fx.cols, null, { shape: fx.shape, orientations: "cols" });
  const mxOnes = show(await Parallel.matVec(rowsOnly, xa));
  const mtyOnes = show(await Parallel.matVec(colsOnly, ya, { transpose: true }));
  const both = await Scalar.fromBigints(x.concat(y));
  const same = await Parallel.matVec(await Parallel.sparseMatrix(fx.rows, fx.cols, values, { shape: fx.shape }), both, { out: both, firstOut: nCols });
  const intoRange = show(both);
  const info = N.matrixInfo(Curve._ctx, m.handle);
  const d = N.descriptorSizes("matrix");
  const sizes = d.sparse === 56 && d.matvec === 32 && d.matRows === 1 && d.matCols === 2 && d.matvecTranspose === 1 &&
    N.descriptorSizes().sparse === undefined;
  let refused = 0;
  for (const bad of [() => Parallel.sparseMatrix([nRows], [0], null, { shape: fx.shape }), () => Parallel.matVec(rowsOnly, ya, { transpose: true }),
                     () => Parallel.matVec(rowsOnly, both, { out: both, firstOut: nCols - 1 }),
                     () => Parallel.sparseMatrix([0], [0], [curveParams.order], { shape: fx.shape })]) {
    try {
      await bad();
    } catch (e) {
      if (/sparseMatrix|matVec/.test(e.message)) refused++;
    }
  }
  m.free();
  Curve.close();
  console.log(JSON.stringify({ mx, mty, mxOnes, mtyOnes, intoRange, info, sizes, refused: refused === 4 && same === both && m.handle === null }));
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
