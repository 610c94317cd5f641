// TypeScript declarations for js/parallel.mjs -- the shape of the reference's src/parallel.ts exports.
export type CurveParams = {
  label: string; curveId: number; kind: "weierstrass" | "twisted-edwards"; feBytes: number;
  modulus: bigint; order: bigint; cofactor: bigint; a?: bigint; b?: bigint; d?: bigint;
  generator: { x: bigint; y: bigint }; endomorphism?: { lambda: bigint; beta: bigint };
};
export type BigintPoint = { x: bigint; y: bigint; isZero?: boolean };
export interface NttOptions { inverse?: boolean; shift?: bigint | null; root?: bigint | null; nIn?: number | null; count?: number;
                              first?: number; out?: DeviceArray | null; firstOut?: number }
/** the checked arguments of Parallel.ntt (host only) */
/** compressed / sign of pointsFromBytes and pointsToCompressedBytes, checked before any call */
export function compressedArgs(who: string, compressed?: boolean, sign?: "largest" | "parity", montgomery?: boolean): { compressed: boolean; sign: "largest" | "parity" };
export function nttArgs(x: { handle: unknown; n: number; kind: string }, logN: number, options: NttOptions | undefined, order: bigint):
  { logN: number; flags: number; nIn: number; count: number; first: number; firstOut: number; root: bigint | null; shift: bigint | null };
/** the limits of the multilinear calls (include/msmz.h) */
export const MLE_MAX_VARS: 31, SUMCHECK_MAX_TABLES: 6, SUMCHECK_MAX_DEGREE: 4, SUMCHECK_MAX_TERMS: 8;
type ScalarsLike = { handle: unknown; n: number; kind: string };
export interface MleBindOptions { nVars?: number | null; count?: number; low?: boolean; first?: number; out?: DeviceArray | null; firstOut?: number }
export interface SumcheckOptions { nVars?: number | null; low?: boolean }
/** a term of a sumcheck: [coefficient or null (1), mask], bit j of the mask making table j a factor (at most 4) */
export type SumcheckTerm = [bigint | null, number];
/** the checked arguments of Parallel.eqTable / evaluateMle / bindMle / sumcheckRound (host only) */
export function eqTableArgs(point: bigint[], scale: bigint, order: bigint): { nVars: number; scale: bigint | null };
export function mleEvalArgs(f: ScalarsLike, point: bigint[], options: { first?: number } | undefined, order: bigint): { nVars: number; first: number };
export function mleBindArgs(f: ScalarsLike, r: bigint, options: MleBindOptions | undefined, order: bigint):
  { nVars: number; count: number; flags: number; first: number; firstOut: number; n: number };
export function sumcheckRoundArgs(tables: (ScalarsLike | [ScalarsLike, number])[], terms: SumcheckTerm[], options: SumcheckOptions | undefined, order: bigint):
  { tables: [ScalarsLike, number][]; nVars: number; terms: SumcheckTerm[]; flags: number; degree: number };
export interface SumcheckStepOptions { nVars?: number | null; out?: (DeviceArray | [DeviceArray, number])[] | null; low?: boolean }
/** the checked arguments of Parallel.sumcheckStep (host only): those of sumcheckRound, r, the destinations and their overlap rules */
export function sumcheckStepArgs(tables: (ScalarsLike | [ScalarsLike, number])[], terms: SumcheckTerm[], r: bigint,
  options: { nVars?: number | null; out?: (ScalarsLike | [ScalarsLike, number])[] | null; low?: boolean } | undefined, order: bigint):
  { tables: [ScalarsLike, number][]; out: [ScalarsLike, number][] | null; nVars: number; terms: SumcheckTerm[]; flags: number; degree: number };
/** the checked arguments of Parallel.innerProducts (host only), in the order of msmz_scalars_dot_many */
export function dotManyArgs(rows: (ScalarsLike | [ScalarsLike, number])[], cols: (ScalarsLike | [ScalarsLike, number])[], n?: number | null,
  options?: { out?: ScalarsLike | null; firstOut?: number }, who?: string):
  { rows: [ScalarsLike, number][]; cols: [ScalarsLike, number][]; n: number; firstOut: number };
/** a resident sparse matrix (msmz_matrix_create) */
export interface SparseMatrix { readonly shape: [number, number]; readonly nnz: number; readonly orientations: "rows" | "cols" | "both"; readonly kind: "matrix"; free(): void }
export interface SparseMatrixOptions { shape: [number, number]; orientations?: "rows" | "cols" | "both"; firstValue?: number }
export interface MatVecOptions { firstX?: number; transpose?: boolean; out?: DeviceArray | null; firstOut?: number }
/** the checked arguments of Parallel.sparseMatrix / matVec (host only) */
export function sparseMatrixArgs(rows: number[] | Uint32Array, cols: number[] | Uint32Array, values: ScalarsLike | null, options: SparseMatrixOptions):
  { rows: Uint8Array; cols: Uint8Array; nnz: number; shape: [number, number]; flags: number; firstValue: number };
export function matVecArgs(matrix: { handle: unknown; shape: number[]; orientations: string; kind: string }, x: ScalarsLike, options?: MatVecOptions): { n: number; flags: number };
export interface LookupOptions { firstColumn?: number; n?: number | null; firstTable?: number; tableN?: number | null; out?: DeviceArray | null; firstOut?: number; positions?: boolean }
export interface ExprOptions { n?: number | null; out?: DeviceArray | null; firstOut?: number }
export type ExprColumn = ScalarsLike | [ScalarsLike, number];
export type ExprFactor = number | [number, number];
export type ExprTerm = [bigint | null, ExprFactor[]];
/** the limits of Parallel.evaluateExpression (include/msmz.h MSMZ_EXPR_MAX_*) */
export const EXPR_MAX_COLUMNS: number, EXPR_MAX_TERMS: number, EXPR_MAX_DEGREE: number, EXPR_MAX_OPERANDS: number;
/** the checked arguments of Parallel.evaluateExpression (host only) */
export function exprArgs(columns: ExprColumn[], terms: ExprTerm[], options: ExprOptions | undefined, order: bigint):
  { columns: [ScalarsLike, number][]; terms: [bigint | null, [number, number][]][]; n: number };
export interface LookupInfo { missing: number; firstMissing: number | null; distinct: number; positions?: Uint32Array }
/** the checked arguments of Parallel.lookupMultiplicities (host only) */
export function lookupArgs(column: ScalarsLike, table: ScalarsLike, options?: LookupOptions): { n: number; tableN: number };
export interface DeviceArray extends Array<DeviceArray> { readonly n: number; readonly kind: "points" | "scalars" | "precomputed";
  /** precomputed point sets only (msmz_precomputed_info) */
  readonly info?: { c: number; glv: number; factor: number; K: number; records: number; scalarBits: number }; free(): void }
/** scalarBits: every scalar of the call is below 2^scalarBits (0 / absent = no bound); the windows are sized for it and a
 * scalar that breaks it fails the call */
export type MsmOptions = { c?: number; glv?: boolean | number; useSafeAdditions?: boolean; reduceAffine?: boolean; scalarBits?: number };
export type MsmResult = { result: BigintPoint; log: any[][]; stats: Record<string, any> };
export type CheckResult = { ok: boolean; offCurve: number; offSubgroup: number; firstBad: number | null; verdicts: Uint8Array | null };
export interface ParallelApi {
  randomPointsFast(n: number, options?: { seed?: bigint | number }): Promise<DeviceArray>;
  randomScalars(n: number, options?: { seed?: bigint | number }): Promise<DeviceArray>;
  pointsFromBytes(bytes: Uint8Array, n?: number, isInf?: Uint8Array): Promise<DeviceArray>;
  /** coordinates as 64-bit-limb Montgomery residues v * 2^(8 feBytes) mod p, converted on the GPU */
  pointsFromBytes(bytes: Uint8Array, n: number | undefined, options: { montgomery?: boolean; isInf?: Uint8Array }): Promise<DeviceArray>;
  /** compressed records of feBytes bytes: one coordinate (x; y on the twisted Edwards curve) with the sign of the other in
   * bit 7 of the last byte; sign "largest" (default): the canonical value is above (p - 1) / 2, "parity": it is odd.  The
   * GPU recovers the other coordinate; a record that is no point throws with code "7" */
  pointsFromBytes(bytes: Uint8Array, n: number | undefined, options: { compressed: true; sign?: "largest" | "parity"; isInf?: Uint8Array }): Promise<DeviceArray>;
  /** points [first, first + count) as compressed records; a point at infinity is an all-zero record with isInf 1 */
  pointsToCompressedBytes(points: DeviceArray, options?: { first?: number; count?: number; sign?: "largest" | "parity" }): Promise<{ records: Uint8Array; isInf: Uint8Array }>;
  scalarsFromBytes(bytes: Uint8Array, n?: number): Promise<DeviceArray>;
  /** `width` bytes per scalar on the wire (4..32, a multiple of 4); montgomery: 32-byte records v * 2^256 mod q */
  scalarsFromBytes(bytes: Uint8Array, n: number | undefined, options: { width?: number; montgomery?: boolean }): Promise<DeviceArray>;
  /** entries [first, first + n) as n * width little-endian bytes (the host route of msmz_export_scalars); a scalar that does
   * not fit `width` bytes throws with code "6"; montgomery: 32-byte records v * 2^256 mod q in 64-bit limbs */
  scalarsToBytes(scalars: DeviceArray, options?: { first?: number; n?: number; width?: number; montgomery?: boolean }): Promise<Uint8Array>;
  /** points [first, first + n) as x || y records (montgomery: coordinates v * 2^(8 feBytes) mod p in 64-bit limbs) and their
   * infinity flags (the host route of msmz_export_points); a point at infinity is an all-zero record with isInf 1 */
  pointsToBytes(points: DeviceArray, options?: { first?: number; n?: number; montgomery?: boolean }): Promise<{ records: Uint8Array; isInf: Uint8Array }>;
  /** pointer-style routes of src/parallel.ts:89-133: pointers are numbers in a virtual address space */
  getPointer(size: number): Promise<number>;
  getScalarPointer(size: number): Promise<number>;
  pointsFromBytes(pointPtr: number, pointInputPtr: number, n: number): Promise<void>;
  scalarsFromBytes(scalarPtr: number, scalarInputPtr: number, n: number): Promise<void>;
  msm(scalars: DeviceArray | Uint8Array | number, points: DeviceArray | number, n: number, verbose?: boolean, options?: MsmOptions): Promise<MsmResult>;
  msmUnsafe(scalars: DeviceArray | Uint8Array | number, points: DeviceArray | number, n: number, verbose?: boolean, options?: MsmOptions): Promise<MsmResult>;
  /** fixed-base precomputation: the result goes wherever `points` is taken (factor 0 = all windows in one bucket set) */
  precomputePoints(points: DeviceArray, n: number, options?: { c?: number; glv?: boolean | number; scalarBits?: number }, factor?: number): Promise<DeviceArray>;
  /** are points [first, first + n) on the curve and (subgroup, the default) in the prime-order subgroup?  verdicts: one
   * byte per point, bit 0 = not on the curve, bit 1 = on the curve but outside the subgroup */
  checkPoints(points: DeviceArray, n?: number, options?: { subgroup?: boolean; first?: number; verdicts?: boolean }): Promise<CheckResult>;
  /** a new point array: out[i] = [s_i] points[firstPoint + i] (+ addend[firstAddend + i]); scalars: a resident scalar
   * array or one bigint below the group order for every point; addend may be `points` itself (an IPA fold);
   * scalarBits: every scalar is below 2^scalarBits (the chain walks that many bits); subgroup: the caller vouches that
   * every point lies in the prime-order subgroup (the Weierstrass curves then run the GLV chain) */
  mulPoints(scalars: DeviceArray | bigint, points: DeviceArray, n?: number,
            options?: { addend?: DeviceArray | null; firstPoint?: number; firstScalar?: number; firstAddend?: number;
                        scalarBits?: number; subgroup?: boolean }): Promise<DeviceArray>;
  /** a new point array: out[i] = [scalars[firstScalar + i]] B for ONE base B -- null (the curve's generator), an affine
   * point, or point `baseIndex` of a resident point array -- from a window table of multiples of B; scalarBits: every
   * scalar of the range is below 2^scalarBits */
  fixedBaseMul(scalars: DeviceArray, n?: number,
               options?: { base?: DeviceArray | { x: bigint; y: bigint; isZero?: boolean } | null; baseIndex?: number;
                           firstScalar?: number; scalarBits?: number }): Promise<DeviceArray>;
  /** out[firstOut + i] = a_i x[firstX + i] (+ b_i y[firstY + i]) mod the group order; a, b: one bigint for every entry or
   * a resident scalar array; without `out` a new array, with it that range is overwritten (it may be an input's range
   * exactly, or apart from it) */
  combineScalars(a: DeviceArray | bigint, x: DeviceArray, b?: DeviceArray | bigint | null, y?: DeviceArray | null, n?: number,
                 options?: { firstX?: number; firstY?: number; out?: DeviceArray | null; firstOut?: number; firstA?: number; firstB?: number }): Promise<DeviceArray>;
  /** sum_i x[firstX + i] y[firstY + i] mod the group order (y null: the sum of x) */
  innerProduct(x: DeviceArray, y?: DeviceArray | null, n?: number, options?: { firstX?: number; firstY?: number }): Promise<bigint>;
  /** a new scalar array: entry i = base ratio^i mod the group order */
  scalarPowers(ratio: bigint, n: number, base?: bigint): Promise<DeviceArray>;
  /** every inner product of 1 to 128 row vectors with 1 to 8 column vectors in one call (msmz_scalars_dot_many):
   * result[r][c] = sum_i rows[r][i] cols[c][i]; with `out` the values go row-major into out[firstOut ..] and `out` comes back */
  innerProducts(rows: (DeviceArray | [DeviceArray, number])[], cols: (DeviceArray | [DeviceArray, number])[], n?: number | null): Promise<bigint[][]>;
  innerProducts(rows: (DeviceArray | [DeviceArray, number])[], cols: (DeviceArray | [DeviceArray, number])[], n: number | null,
    options: { out: DeviceArray; firstOut?: number }): Promise<DeviceArray>;
  /** result[r][c] = p_r(z_c) for coefficient vectors polys[r] and 1 to 8 points: one scalarPowers per point, one innerProducts call */
  evaluatePolynomials(polys: (DeviceArray | [DeviceArray, number])[], points: bigint[], n?: number | null): Promise<bigint[][]>;
  /** y_i = a_i y_(i-1) + b_i mod the group order from y_(-1) = init (reverse: y_i = a_i y_(i+1) + b_i from y_n = init);
   * a: a resident scalar array, one bigint for every entry or null (1); b: a resident scalar array or null; entry i of the
   * result is y_i, with `exclusive` the value before the step at i -> [the array written, the final y] */
  scalarRecurrence(a: DeviceArray | bigint | null, b: DeviceArray | null, n?: number,
                   options?: { init?: bigint | null; reverse?: boolean; exclusive?: boolean; firstA?: number; firstB?: number;
                               out?: DeviceArray | null; firstOut?: number }): Promise<[DeviceArray, bigint]>;
  /** running products -> [array, the full product]; exclusive: entry 0 is 1 */
  prefixProducts(x: DeviceArray, n?: number, options?: { exclusive?: boolean; init?: bigint | null; reverse?: boolean; first?: number;
                                                          out?: DeviceArray | null; firstOut?: number }): Promise<[DeviceArray, bigint]>;
  /** running sums -> [array, the full sum] */
  prefixSums(x: DeviceArray, n?: number, options?: { exclusive?: boolean; init?: bigint | null; reverse?: boolean; first?: number;
                                                      out?: DeviceArray | null; firstOut?: number }): Promise<[DeviceArray, bigint]>;
  /** (p(X) - p(z)) / (X - z) -> [the quotient's n coefficients (the top one 0), p(z)] */
  divideByLinear(p: DeviceArray, z: bigint, n?: number, options?: { first?: number }): Promise<[DeviceArray, bigint]>;
  /** out[firstOut + i] = x[first + i]^-1 mod the group order, 0 -> 0 -> [the array written, the number of zeros] */
  invertScalars(x: DeviceArray, n?: number, options?: { first?: number; out?: DeviceArray | null; firstOut?: number }): Promise<[DeviceArray, number]>;
  /** `count` number-theoretic transforms of length 2^logN over resident scalar arrays, natural order in and out
   * (msmz_scalars_ntt); returns the array written */
  ntt(x: DeviceArray, logN: number, options?: NttOptions): Promise<DeviceArray>;
  /** Multilinear polynomials over resident scalar arrays (include/msmz.h msmz_scalars_eq_table / _mle_eval / _mle_bind /
   * _sumcheck_round).  A polynomial in v variables is 2^v consecutive entries, entry i its value at the bits of i,
   * variable 0 the lowest bit; eq(r, i) = prod_j (b_j r_j + (1 - b_j)(1 - r_j)).  eqTable: a new array, entry i =
   * scale eq(point, i) (at most 31 variables; [] gives the one entry scale). */
  eqTable(point: bigint[], scale?: bigint): Promise<DeviceArray>;
  /** f(point) = sum_i f[first + i] eq(point, i); the table is not made */
  evaluateMle(f: DeviceArray, point: bigint[], options?: { first?: number }): Promise<bigint>;
  /** binds the high variable of `count` tables of 2^nVars entries to r: out_i = f_i + r (f_(i+h) - f_i), h = 2^(nVars-1);
   * low: variable 0, out_i = f_(2i) + r (f_(2i+1) - f_(2i)).  `out` may be `f` only for one table, the high variable and
   * firstOut == first (the low half is overwritten), or a range apart from the source.  Returns the array written. */
  bindMle(f: DeviceArray, r: bigint, options?: MleBindOptions): Promise<DeviceArray>;
  /** the round polynomial g(0) .. g(d) of a sumcheck over sum_i sum_T c_T prod_(j in T) tables[j][i]: 1 to 6 tables
   * (arrays or [array, first] pairs), 1 to 8 terms of at most 4 factors, d the most factors of a term; the round sums
   * out the high variable, with `low` variable 0 */
  sumcheckRound(tables: (DeviceArray | [DeviceArray, number])[], terms: SumcheckTerm[], options?: SumcheckOptions): Promise<bigint[]>;
  /** one step of a sumcheck prover (msmz_scalars_sumcheck_step): binds every table to r as bindMle does and returns the
   * polynomial sumcheckRound gives over the bound tables; without `out` in place (high order only); nVars 1: the final claim */
  sumcheckStep(tables: (DeviceArray | [DeviceArray, number])[], terms: SumcheckTerm[], r: bigint, options?: SumcheckStepOptions):
    Promise<{ degree: number; values: bigint[] }>;
  /** a whole sumcheck on the prover's side: one sumcheckRound, then one sumcheckStep per challenge = await challenge(values);
   * the tables are consumed (in place, or with `low` through one scratch array per table that is freed again) */
  sumcheckProve(tables: (DeviceArray | [DeviceArray, number])[], terms: SumcheckTerm[], nVars: number | null,
    challenge: (values: bigint[]) => bigint | Promise<bigint>, options?: { low?: boolean }): Promise<{ polys: bigint[][]; challenges: bigint[]; claim: bigint }>;
  /** a resident sparse matrix from triples (rows[k], cols[k], values[k]) in any order, duplicates adding up
   * (msmz_matrix_create); values: a resident scalar array, bigints (uploaded first) or null (every value is 1) */
  sparseMatrix(rows: number[] | Uint32Array, cols: number[] | Uint32Array, values: DeviceArray | bigint[] | null, options: SparseMatrixOptions): Promise<SparseMatrix>;
  /** out_i = sum over the non-zeros (i, j, v) of v x[firstX + j] mod the group order, with `transpose` over (j, i, v)
   * (msmz_matrix_mul); the destination may not meet the x range.  Returns the array written. */
  matVec(matrix: SparseMatrix, x: DeviceArray, options?: MatVecOptions): Promise<DeviceArray>;
  /** the multiplicities of a column in a table (msmz_scalars_lookup): m[j] = #{i : column[i] = table[j]} at the first
   * index of each table value, 0 at later duplicates; a column entry in no table is counted in info.missing, not refused.
   * The destination may meet neither input range. */
  lookupMultiplicities(column: DeviceArray, table: DeviceArray, options?: LookupOptions): Promise<[DeviceArray, LookupInfo]>;
  /** a sum of products of rotated columns, entry by entry (msmz_scalars_expr): out[i] = sum_T c_T prod_f
   * column_f[(i + rot_f) mod n]; `out` may be a column read at rotation 0 only (in place) or apart from every column read */
  evaluateExpression(columns: (DeviceArray | [DeviceArray, number])[], terms: ExprTerm[], options?: ExprOptions): Promise<DeviceArray>;
  /** the default primitive 2^logN-th root of unity of the scalar field (msmz_scalars_root_of_unity) */
  rootOfUnity(logN: number): bigint;
  msmBatch(scalarsList: DeviceArray | Uint8Array[], points: DeviceArray, n: number, options?: MsmOptions & { batch?: number }): Promise<BigintPoint[]>;
  msmBatchUnsafe(scalarsList: DeviceArray | Uint8Array[], points: DeviceArray, n: number, options?: MsmOptions & { batch?: number }): Promise<BigintPoint[]>;
  /** one MSM per segment [firstPoint, firstScalar, n] of one resident scalar array and one resident point array */
  msmSegments(scalars: DeviceArray, points: DeviceArray, segments: [number, number, number][], options?: MsmOptions): Promise<BigintPoint[]>;
  msmSegmentsUnsafe(scalars: DeviceArray, points: DeviceArray, segments: [number, number, number][], options?: MsmOptions): Promise<BigintPoint[]>;
  msmProjective?(scalars: DeviceArray | Uint8Array, points: DeviceArray, n: number, options?: MsmOptions): Promise<MsmResult>;
}
export interface MsmCurve {
  params: CurveParams; Parallel: ParallelApi;
  Field: { sizeField: number; memoryBytes: { set(bytes: Uint8Array, ptr: number): void }; isEqual(a: number, b: number): boolean;
           local: { getPointers(n: number): number[]; getPointer(size: number): number } };
  Scalar: { sizeField: number; memoryBytes: { set(bytes: Uint8Array, ptr: number): void }; writeBigint(ptr: number, s: bigint): void;
            modulus: bigint; sizeInBits: number; readBigint(a: DeviceArray, i?: number): bigint; toBigints(a: DeviceArray, first?: number, count?: number): bigint[]; fromBigints(s: bigint[]): Promise<DeviceArray> };
  Affine: { size: number; toBigint(p: BigintPoint | number): BigintPoint; writeBigints(ptr: number, points: BigintPoint[]): number; toBigints(a: DeviceArray, first?: number, count?: number): BigintPoint[]; fromBigints(p: BigintPoint[]): Promise<DeviceArray> };
  Projective: { toAffine(scratch: unknown, affPtr: number | null, result: BigintPoint): BigintPoint; toBigint(r: BigintPoint): BigintPoint };
  pointAdd(a: BigintPoint, b: BigintPoint): BigintPoint; close(): void;
}
/** n = number of GPUs a curve context drives (inputs split over them); deviceId = first GPU or an explicit list */
export function startThreads(n?: number, deviceId?: number | number[]): Promise<number | number[]>;
export function stopThreads(): Promise<void>;
export const Weierstraß: { create(params: CurveParams): Promise<MsmCurve> };
export const Weierstrass: { create(params: CurveParams): Promise<MsmCurve> };
export const TwistedEdwards: { create(params: CurveParams): Promise<MsmCurve> };
