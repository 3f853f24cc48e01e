"""Host side of `jx fvlmm2`: the interaction-file grammar, the code tables of a SNP pair, the Benjamini-Hochberg adjustment, the
number formats and the table writers.  The device side is `janusx.fvlmm2_pairs_packed` (csrc/k_fvlmm2.hip); for `-screen` (the
variants by genotype class, the chi^2 quantile, the residual, the screen table) `janusx.fvlmm2_screen_packed` (csrc/k_pairscreen.hip).

The rules are those of the reference's script (python/janusx/script/fvlmm2.py), restated: the strings a user meets -- the grammar,
the skip reasons, the error texts, the column names -- are the reference's, the code is this project's.

A decoded row takes four values, one per 2-bit code (`bed_packed_decode_rows_f32`: [0, mean, 1, 2] or flipped, mean = 2 maf), so a
literal is a function of one code and every combo value a function of the two codes of a pair: a 4 x 4 f32 table."""
from __future__ import annotations

import csv
import math
import re
import string
from typing import NamedTuple

import numpy as np

OPS = ("*", "&", "|", "^")
AMONG_MAX_NAMES = 4096
NO_EXPRESSIONS = "No valid interaction expressions remain after variant lookup/filtering."
OUTPUT_COLUMNS = ("chrom", "pos", "combo_id", "combo_af", "unit_name", "beta_combo_joint", "se_combo_joint", "p_combo_joint",
                  "p_combo_joint_fdr", "p_lit1_joint", "p_lit2_joint")
REASON_INVALID = "invalid_expression"
REASON_NEGATED_PRODUCT = "negated_literals_not_supported_for_multiplicative_interaction"


class PairSpec(NamedTuple):
    """One resolved expression: the two active rows, the operator, the negations, and the names as they are printed."""
    row1: int
    row2: int
    op: str
    neg1: bool
    neg2: bool
    expr: str
    snp1: str
    snp2: str


class Skipped(NamedTuple):
    """One line of `.fvlmm2.skip`: where the expression stood, how it is spelled, why it was not tested."""
    line: str
    expr: str
    reason: str


class NameLookupError(LookupError):
    """A SNP name that does not stand for exactly one active row; `reason` is the text of the skip table."""

    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


# ---- names --------------------------------------------------------------------------------------------------------------

def normalize_snp_name(raw_name, chrom, pos):
    """The name of a site; a site without one (empty, '.', 'nan') is called chrom_pos."""
    name = str(raw_name).strip()
    return name if name.lower() not in ("", ".", "nan") else f"{str(chrom).strip()}_{int(pos)}"


def build_name_map(chrom, pos, snp):
    """-> (the name of every active row, index {name: [rows]}).  A row answers to its name and to chrom_pos."""
    names = [normalize_snp_name(s, c, p) for s, c, p in zip(snp, chrom, pos)]
    index = {}
    for row, (name, c, p) in enumerate(zip(names, chrom, pos)):
        for key in dict.fromkeys((name, f"{c}_{int(p)}")):            # once when the two spellings are the same
            index.setdefault(key, []).append(row)
    return names, index


def resolve_snp_token(token, index):
    """The one active row a name stands for; NameLookupError otherwise.  The reference raises a KeyError for an unknown name and
    prints its `str`, which is the repr of the message: the reason keeps those quotes."""
    rows = index.get(str(token).strip())
    if not rows:
        raise NameLookupError(repr(f"SNP token '{token}' was not found among active filtered variants."))
    if len(rows) != 1:
        raise NameLookupError(f"SNP token '{token}' is ambiguous after filtering; matched {len(rows)} active rows.")
    return rows[0]


def split_literal_token(token):
    """'!!rs1' -> ('rs1', False), '!rs1' -> ('rs1', True): an odd count of leading '!' negates the literal."""
    text = str(token).strip()
    if not text:
        raise ValueError("Literal token is empty.")
    name = text.lstrip("!" + string.whitespace)
    if not name:
        raise ValueError("Literal token has no SNP name after '!'.")
    bangs = text[:len(text) - len(name)].count("!")
    return name, bangs % 2 == 1


def _split_expression(token):
    """'a&b' -> ('a', '&', 'b'), or None: exactly one operator character with something on both sides."""
    at = [k for k, ch in enumerate(token) if ch in OPS]
    if len(at) != 1 or at[0] in (0, len(token) - 1):
        return None
    return token[:at[0]], token[at[0]], token[at[0] + 1:]


def _spelled(name, negated):
    return ("!" if negated else "") + name


def _resolve_expression(token, index):
    """A PairSpec, or (expr, reason) for the skip table."""
    parts = _split_expression(token)
    if parts is None:
        return token, REASON_INVALID
    left, op, right = parts
    try:
        (snp1, neg1), (snp2, neg2) = split_literal_token(left), split_literal_token(right)
    except ValueError as e:
        return f"{left}{op}{right}", str(e)
    expr = _spelled(snp1, neg1) + op + _spelled(snp2, neg2)
    if op == "*" and (neg1 or neg2):
        return expr, REASON_NEGATED_PRODUCT
    try:
        return PairSpec(resolve_snp_token(snp1, index), resolve_snp_token(snp2, index), op, neg1, neg2, expr, snp1, snp2)
    except NameLookupError as e:
        return expr, e.reason


def parse_interaction_file(path, index):
    """One expression per line, the line's first word; blank lines and lines that begin with '#' do not count
    -> (list of PairSpec, list of Skipped with the 1-based line number)."""
    specs, skipped = [], []
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        for number, text in enumerate(fh, start=1):
            words = text.split()
            if not words or words[0].startswith("#"):
                continue
            got = _resolve_expression(words[0], index)
            if isinstance(got, PairSpec):
                specs.append(got)
            else:
                skipped.append(Skipped(str(number), *got))
    return specs, skipped


def read_among_names(path):
    """`-among` file (extension): one SNP name per line (its first word), '#' and blank lines passed over, at most 4096 names."""
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        names = [w[0] for w in (line.split() for line in fh) if w and not w[0].startswith("#")]
    if len(names) > AMONG_MAX_NAMES:
        raise ValueError(f"-among: at most {AMONG_MAX_NAMES} SNP names, got {len(names)}")
    return names


def among_specs(names, index, row_names, op="*"):
    """All unordered pairs among the named SNPs in ascending active-row order, one operator (extension) -> (specs, skipped).
    Names that resolve to the same row count once; a name that does not resolve is skipped with the parser's reason."""
    if op not in OPS:
        raise ValueError(f"Unsupported interaction operator: {op}")
    rows, skipped = set(), []
    for k, name in enumerate(names, start=1):
        try:
            rows.add(resolve_snp_token(name, index))
        except NameLookupError as e:
            skipped.append(Skipped(f"among:{k}", str(name), e.reason))
    order = sorted(rows)
    specs = [PairSpec(a, b, op, False, False, f"{row_names[a]}{op}{row_names[b]}", row_names[a], row_names[b])
             for i, a in enumerate(order) for b in order[i + 1:]]
    return specs, skipped


# ---- tables -------------------------------------------------------------------------------------------------------------

# the dual-dosage XOR of two hard calls: equal calls give 0 (two hets: 1), a het on one side gives 1, opposite homozygotes 2
_XOR3 = np.array([[0, 1, 2],
                  [1, 1, 1],
                  [2, 1, 0]], dtype=np.float32)


def literal_values(lut, neg):
    """The literal of every code: the hard call nearest to the decoded value (ties to even, so a mean of 0.5 is 0 and 1.5 is 2),
    counted from the other allele (2 - call) when negated.  lut (R, 4) f32, neg (R) bool -> (R, 4) f32."""
    call = np.rint(np.clip(np.asarray(lut, dtype=np.float32), 0, 2))
    flipped = np.asarray(neg, dtype=bool)[:, None]
    return np.where(flipped, 2 - call, call).astype(np.float32)


def pair_tables(lut1, lut2, ops, neg1, neg2):
    """Tables of R pairs: lut1, lut2 (R, 4) f32 decoded value by code; ops R operators; neg1, neg2 (R) bool
    -> (tab (R, 16) f32 with tab[r][4 c1 + c2] = combo value, pos (R) uint32: bit c1 literal 1 > 0, bit 4 + c2 literal 2 > 0,
    bit 8 + 4 c1 + c2 combo > 0).  '*' is the f32 product of the decoded values and takes no negation; '&' is the smaller and '|'
    the larger of the two literals; '^' is `_XOR3`."""
    lut1 = np.ascontiguousarray(lut1, dtype=np.float32).reshape(-1, 4)
    lut2 = np.ascontiguousarray(lut2, dtype=np.float32).reshape(-1, 4)
    ops = np.asarray(list(ops), dtype="U1")
    neg1, neg2 = np.asarray(neg1, dtype=bool).ravel(), np.asarray(neg2, dtype=bool).ravel()
    r = lut1.shape[0]
    if not (lut2.shape[0] == ops.shape[0] == neg1.shape[0] == neg2.shape[0] == r):
        raise ValueError("pair_tables: one entry per pair in every argument")
    unknown = sorted(set(ops.tolist()) - set(OPS))
    if unknown:
        raise ValueError(f"Unsupported interaction operator: {unknown[0]}")
    if np.any((ops == "*") & (neg1 | neg2)):
        raise ValueError("Negated literals are not supported for multiplicative interaction '*'.")
    if not (np.isfinite(lut1).all() and np.isfinite(lut2).all()):
        raise ValueError("pair_tables: decoded values must be finite")
    lit1, lit2 = literal_values(lut1, neg1), literal_values(lut2, neg2)
    # (R, 4, 4) grids over (c1, c2)
    a, b = lit1[:, :, None], lit2[:, None, :]
    grids = {"*": lut1[:, :, None] * lut2[:, None, :],
             "&": np.minimum(a, b),
             "|": np.maximum(a, b),
             "^": _XOR3[lit1.astype(np.intp)[:, :, None], lit2.astype(np.intp)[:, None, :]]}
    tab = np.empty((r, 16), dtype=np.float32)
    for op, grid in grids.items():
        sel = ops == op
        tab[sel] = grid.reshape(r, 16)[sel]
    bits = np.concatenate([lit1 > 0, lit2 > 0, tab > 0], axis=1)
    pos = (bits * (np.uint32(1) << np.arange(24, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    return tab, pos


# ---- multiple testing and formats ---------------------------------------------------------------------------------------

def bh_adjust(pvalues, n_tests=None):
    """Benjamini-Hochberg step-up over the entries that are finite and not negative (values above 1 count as 1); the others stay
    NaN.  The hypothesis count is the number of such entries, or `n_tests` when that is larger.  Equal p-values keep their order."""
    p = np.asarray(pvalues, dtype=np.float64).ravel()
    adjusted = np.full(p.shape, np.nan)
    where = np.flatnonzero(np.isfinite(p) & (p >= 0.0))
    if where.size == 0:
        return adjusted
    q = np.minimum(p[where], 1.0)
    ascending = np.argsort(q, kind="stable")
    hypotheses = float(max(where.size, int(n_tests or 0)))
    scaled = q[ascending] * (hypotheses / np.arange(1.0, where.size + 1.0))       # p_(k) m / k
    # the adjusted value of rank k is the least scaled value at rank k or beyond; it is never below p_(k) itself, since m >= k
    step_up = np.minimum.accumulate(scaled[::-1])[::-1]
    adjusted[where[ascending]] = np.minimum(step_up, 1.0)
    return adjusted


def _finite(value):
    try:
        v = float(value)
    except (TypeError, ValueError):
        return None
    return v if math.isfinite(v) else None


def format_fixed4(value):
    v = _finite(value)
    return "NA" if v is None else f"{v:.4f}"


def format_sci4(value):
    """Five significant digits in scientific form without padding: 1.2e-5 for 0.000012, 1e0 for 1, 0e0 for 0; NA when not finite."""
    v = _finite(value)
    if v is None:
        return "NA"
    if v == 0.0:
        return "0e0"
    mantissa, _, exponent = f"{v:.4e}".partition("e")          # the rounding to five digits may carry into the exponent
    return f"{float(mantissa):.5g}e{int(exponent)}"


def format_pos_int(value):
    v = _finite(value)
    return "NA" if v is None else str(round(v))


def format_row(chrom, pos, combo_id, combo_af, unit_name, beta_c, se_c, p_c, p_fdr, p1, p2):
    unit = str(unit_name).strip()
    if unit.lower() in ("", "nan"):
        unit = "."
    return [str(chrom), format_pos_int(pos), str(combo_id), format_fixed4(combo_af), unit, format_fixed4(beta_c),
            format_fixed4(se_c), format_sci4(p_c), format_sci4(p_fdr), format_sci4(p1), format_sci4(p2)]


def write_table(path, chrom, pos, combo_id, combo_af, joint, fdr, keep=None):
    """The compact 11-column table.  joint (R, 9) = (beta, se, p) of literal 1, literal 2, combo; `keep` (R) bool: the rows to
    write (None: all) -> rows written.  No unit names exist on this route: the column holds '.'."""
    joint = np.asarray(joint, dtype=np.float64).reshape(-1, 9)
    rows = range(joint.shape[0]) if keep is None else np.nonzero(np.asarray(keep, dtype=bool))[0]
    n_out = 0
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\t".join(OUTPUT_COLUMNS) + "\n")
        for r in rows:
            fh.write("\t".join(format_row(chrom[r], pos[r], combo_id[r], combo_af[r], "", joint[r, 6], joint[r, 7], joint[r, 8],
                                          fdr[r], joint[r, 2], joint[r, 5])) + "\n")
            n_out += 1
    return n_out


def write_skip(path, skipped):
    """`{out}.fvlmm2.skip`: line, expr, reason, tab separated with minimal quoting, as a data-frame writer quotes: a reason that
    holds a double quote (an unknown name) is wrapped and its quotes doubled."""
    with open(path, "w", encoding="utf-8", newline="") as fh:
        w = csv.writer(fh, delimiter="\t", lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
        w.writerow(Skipped._fields)
        w.writerows(skipped)


# ---- the pair screen (`-screen`, an extension; device side: janusx.fvlmm2_screen_packed, csrc/k_pairscreen.hip) ---------------

SCREEN_DEFAULT_OPS = "*,&,|,^"
SCREEN_DEFAULT_P = 1e-5
SCREEN_DEFAULT_TOP = 4096           # one device batch of the joint test
SCREEN_MAX_VARIANTS = 16
SCREEN_COLUMNS = ("snp1", "snp2", "combo_id", "n_complete", "stat", "p_screen")


class ScreenVariant(NamedTuple):
    """One combo of the screen by genotype class (hom-ref 0, het 1, hom-alt 2): combo (3, 3)[a][b], lit1 (3)[a], lit2 (3)[b], f64."""
    op: str
    neg1: bool
    neg2: bool
    combo: np.ndarray
    lit1: np.ndarray
    lit2: np.ndarray

    def spelled(self, snp1, snp2):
        """The expression as the interaction parser reads it back."""
        return _spelled(snp1, self.neg1) + self.op + _spelled(snp2, self.neg2)


def variant_tables(op, neg1, neg2):
    """The class tables of one (op, neg1, neg2) on hard calls, by the rules of `pair_tables`: a literal is the call, or 2 - call when
    negated; '&' the smaller, '|' the larger of the literals, '^' `_XOR3`, '*' the product of the calls (no negation)."""
    if op not in OPS:
        raise ValueError(f"Unsupported interaction operator: {op}")
    if op == "*" and (neg1 or neg2):
        raise ValueError("Negated literals are not supported for multiplicative interaction '*'.")
    call = np.arange(3, dtype=np.float64)
    lit1, lit2 = (2.0 - call if neg1 else call), (2.0 - call if neg2 else call)
    a, b = lit1[:, None], lit2[None, :]
    if op == "*":
        combo = a * b
    elif op == "&":
        combo = np.minimum(a, b)
    elif op == "|":
        combo = np.maximum(a, b)
    else:
        combo = _XOR3.astype(np.float64)[lit1.astype(np.intp)[:, None], lit2.astype(np.intp)[None, :]]
    return ScreenVariant(op, bool(neg1), bool(neg2), np.ascontiguousarray(combo, dtype=np.float64), lit1, lit2)


def screen_variants(spec=SCREEN_DEFAULT_OPS):
    """`-screen-ops`: a comma-separated list of operators.  '&' and '|' alone stand for their four negation patterns, '!&', '&!'
    and '!&!' (likewise '|') for one of them; '^' and '*' take no negation.  The default gives 10 variants; at most 16; an entry
    that comes twice counts once -> list of ScreenVariant in the order of the list."""
    out, seen = [], set()
    tokens = [t.strip() for t in str(spec).split(",")]
    if not any(tokens):
        raise ValueError("-screen-ops: no operator given")
    for tok in tokens:
        core = tok.strip("!")
        if core not in OPS or tok not in (core, "!" + core, core + "!", "!" + core + "!"):
            raise ValueError(f"-screen-ops: unsupported entry '{tok}' (operators: {' '.join(OPS)}; '!' before / after '&' or '|')")
        if tok == core:
            patterns = [(False, False), (True, False), (False, True), (True, True)] if core in ("&", "|") else [(False, False)]
        else:
            if core in ("*", "^"):
                raise ValueError(f"-screen-ops: '{core}' takes no negation")
            patterns = [(tok.startswith("!"), tok.endswith("!"))]
        for neg1, neg2 in patterns:
            if (core, neg1, neg2) not in seen:
                seen.add((core, neg1, neg2))
                out.append(variant_tables(core, neg1, neg2))
    if len(out) > SCREEN_MAX_VARIANTS:
        raise ValueError(f"-screen-ops: at most {SCREEN_MAX_VARIANTS} variants, got {len(out)}")
    return out


def variant_array(variants):
    """(V, 15) f64 for the device: combo (9, a major), lit1 (3), lit2 (3) of every variant; a (V, 15) array passes through."""
    if isinstance(variants, np.ndarray):
        return np.ascontiguousarray(variants, dtype=np.float64).reshape(-1, 15)
    return np.array([np.concatenate([np.asarray(v.combo, dtype=np.float64).reshape(9), np.asarray(v.lit1, dtype=np.float64).reshape(3),
                                     np.asarray(v.lit2, dtype=np.float64).reshape(3)]) for v in variants],
                    dtype=np.float64).reshape(-1, 15)


def permute_classes(variant, flip1, flip2):
    """The variant as a flipped row sees it: a flipped row's class a reads the tables at 2 - a."""
    i1 = [2, 1, 0] if flip1 else [0, 1, 2]
    i2 = [2, 1, 0] if flip2 else [0, 1, 2]
    return variant._replace(combo=variant.combo[np.ix_(i1, i2)], lit1=variant.lit1[i1], lit2=variant.lit2[i2])


def chi2_1_pvalue(stat):
    """The upper tail of chi^2_1 (`lm2.chi2_sf`, the project's own code)."""
    from .lm2 import chi2_sf
    return chi2_sf(float(stat), 1.0)


def chi2_1_quantile(p):
    """t with chi2_1_pvalue(t) = p, 0 < p < 1, by bisection on the forward p-value (monotone); the bracket ends where the erfc form
    underflows."""
    p = float(p)
    if not (0.0 < p < 1.0):
        raise ValueError("-screen P must be within (0, 1)")
    lo, hi = 0.0, 1400.0
    if chi2_1_pvalue(hi) >= p:
        return hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if chi2_1_pvalue(mid) > p:
            lo = mid
        else:
            hi = mid
    return hi


def screen_residual(s, xcov_rot, y_rot, u_t, lbd):
    """The GRAMMAR residual of the null fit in sample space and its variance -> (r (n) f64, sigma2):
    r = U W (y~ - X~ b^), W = 1 / (s + lambda), b^ the GLS estimate of the rotated null model; sigma2 = r'r / (n - p_cov).
    s, xcov_rot, y_rot, u_t: host arrays or torch tensors; u_t (n, n) is U^T row-major, so r = u_t' v, taken in row blocks in f64."""
    def host(a):
        return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)
    s, x, y = host(s).ravel(), host(xcov_rot), host(y_rot).ravel()
    n = y.shape[0]
    x = x.reshape(n, -1)
    w = 1.0 / (s + float(lbd))
    xw = x * w[:, None]
    beta = np.linalg.solve(xw.T @ x, xw.T @ y)
    v = w * (y - x @ beta)
    if tuple(u_t.shape) != (n, n):
        raise ValueError("u_t must be (n, n) and row-major U^T")
    r = np.zeros(n, dtype=np.float64)
    step = 2048
    if hasattr(u_t, "detach"):
        import torch
        vt = torch.from_numpy(v).to(u_t.device)
        rt = torch.zeros(n, dtype=torch.float64, device=u_t.device)
        for k0 in range(0, n, step):
            rt += vt[k0:k0 + step] @ u_t[k0:k0 + step].to(torch.float64)
        r = rt.cpu().numpy()
    else:
        for k0 in range(0, n, step):
            r += v[k0:k0 + step] @ np.asarray(u_t[k0:k0 + step], dtype=np.float64)
    dof = n - x.shape[1]
    if dof <= 0:
        raise ValueError("screen_residual: n must exceed the covariate count")
    return r, float(r @ r) / float(dof)


def write_screen_table(path, snp1, snp2, combo_id, n_complete, stat):
    """`{out}.{trait}.fvlmm2.screen.tsv`: one line per kept hit in the order given; p_screen is the chi^2_1 tail of stat (it ranks,
    it does not test) -> lines written."""
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\t".join(SCREEN_COLUMNS) + "\n")
        for a, b, cid, nc, t in zip(snp1, snp2, combo_id, n_complete, stat):
            fh.write("\t".join([str(a), str(b), str(cid), str(int(nc)), format_fixed4(t), format_sci4(chi2_1_pvalue(t))]) + "\n")
    return len(stat)


def trait_label(trait_ref):
    """The trait's name as part of a file name: no path separators; 'trait' when empty."""
    return re.sub(r"[/\\]", "_", str(trait_ref).strip()) or "trait"
