"""Thin `jx gwas` / `jx grm` / `jx gs` command line for the accelerated path.

Flag names, defaults and output file names follow the reference (python/janusx/assoc/workflow.py:6599-7047,
python/janusx/script/grm.py:18-23, 1874-1975, python/janusx/assoc/workflow_model_stream.py:989-994):

  python -m janusx_amd gwas -bfile PREFIX -p PHENO.tsv [-n TRAIT ...] (-lm | -lm2 COVCOL | -lmm | -lmm2 | -fvlmm) [-k 1|2|GRM.npy] [-c COV.tsv]
                            [-maf 0.02] [-geno 0.05] [-het 1.0] [-o OUT] [-force-model]
  python -m janusx_amd gwas -bfile PREFIX -p PHENO.tsv -n T1 -n T2 ... -lm -trait-level [-trait-pmax P] [-c COV.tsv] [-o OUT]
                            (many traits in one pass: traits that share a sample mask are scanned together, one table {out}.lm.tsv)
  python -m janusx_amd gwas -bfile PREFIX -p PHENO.tsv -n T1 -n T2 ... -lmm -trait-level-lmm [-chunksize N] [-warm-start none|chain]
                            [-warm-chain-pieces P] [-force-model] [-trait-pmax P]
                            (traits that share a sample mask share one eigendecomposition and one rotation of every SNP block,
                            one table {out}.lmm.tsv)
  python -m janusx_amd gwas -bfile PREFIX -p PHENO.tsv [-n TRAIT ...] -farmcpu [-q N] [-c COV.tsv] [--farmcpu-iter 30]
                            [--farmcpu-threshold P] [--farmcpu-qtn-bound auto|N] [--farmcpu-nbin 5]
                            [--farmcpu-bin-size 500000,5000000,50000000]
                            (FarmCPU, the classic route: {out}.{trait}.farmcpu.tsv and {out}.{trait}.farmcpu.qtn)
  python -m janusx_amd grm  -bfile PREFIX [-m 1|2] [-maf 0.02] [-geno 0.05] [-o OUT]
  python -m janusx_amd pca  (-bfile PREFIX | -k GRM) [-dim 3] [-maf 0.02] [-geno 0.05] [-rsvd [power] [tol]] [-snps-only] [-o OUT]
  python -m janusx_amd adamixture -bfile PREFIX -k 2..4 [-o OUTDIR] [-prefix NAME] [-maf 0.02] [-geno 0.05] [-seed 42]
                                 [-solver adam-em|adam|auto] [-max-iter 500] [-check 5] [-tol 1e-5] [-snps-only] [-cverror [N]]
                                 (fastpop: same)
  python -m janusx_amd gformat -bfile PREFIX -prune WINDOW STEP R2 [-o OUT | -o DIR/ -prefix NAME]   (LD pruning; WINDOW: 50, 500kb, 100bp)
  python -m janusx_amd gstats -bfile PREFIX [-freq] [-miss] [-het] [-ldsc [WINDOW]] [-o OUT | -o DIR/ -prefix NAME]
                                 (site / sample QC tables and LD scores; WINDOW: 100, 100kb, 0.1mb, 100000b, 10cm; bare -ldsc: 100kb)
  python -m janusx_amd tree -bfile PREFIX -nj [exact] [-maf 0.02] [-geno 0.05] [-het 0.02] [-snps-only] [-o OUT | -o DIR/ -prefix NAME]
                                 [--write-phylip] [--no-fasta]   (neighbour-joining tree: {out}.nwk, {out}.fasta, {out}.phy)
  python -m janusx_amd fvlmm2 -bfile PREFIX -p PHENO.tsv [-n TRAIT ...] (-i PAIRS.txt | -among SNPS.txt [--op '*'] | -screen [P]) [-c COV.tsv] [-k GRM.npy]
                                 [-maf 0.02] [-geno 0.05] [-het 1.0] [-snps-only] [--batch-size 4096] [--n-tests 0] [-pmax P]
                                 [-screen-top 4096] [-screen-ops '*,&,|,^'] [-screen-min-dist BP] [-screen-among SNPS.txt]
                                 [-o OUT | -o DIR/ -prefix NAME]   (joint SNP-pair interaction test at the null lambda:
                                 {out}.{trait}.fvlmm2.tsv, {out}.fvlmm2.skip; -screen: exhaustive pair screen in front of it,
                                 {out}.{trait}.fvlmm2.screen.tsv, whose p_screen ranks and does not test)
  python -m janusx_amd gs   -bfile PREFIX -p PHENO.tsv [-n TRAIT ...] -BLUP [-cv K] [-seed 42] [-k GRM.npy]
  python -m janusx_amd gs   -bfile PREFIX -p PHENO.tsv [-n TRAIT ...] -rrBLUP [-lambda L] [-tol 1e-4] [-max-iter 100] [-cv K]
                            [-maf 0.02] [-geno 0.05] [-o OUT]

Outputs: `{out}.{trait}.lm.tsv` (`gwas -lm`, plain linear model) / `.lm2.tsv` (`gwas -lm2 COVCOL`, SNP-by-covariate interaction scan over the 0-based columns COVCOL of the merged -c table: 0, 0:3, :2, 0,3) / `.lmm.tsv` / `.lmm2.tsv` / `.fvlmm.tsv` / `.splmm2.tsv` (`gwas -splmm-exact [cutoff]`, exact SparseLMM scan) / `.splmm.tsv` (`gwas -splmm [cutoff]`, GRAMMAR-gamma SparseLMM scan); `{out}.cGRM.npy` (method 1) or `.sGRM.npy` (method 2) + `.npy.id`; `{out}.spgrm` + `.spgrm.id` with `grm -sparse [cutoff]`;
`{out}.{trait}.gs.GBLUP.tsv` (sample, observed, predicted, fold) for `gs`; `{out}.eigenvec` + `{out}.eigenval` for `pca`;
`{out}.freq` / `.lmiss` / `.lhet` (chr, pos, value), `{out}.imiss` / `.ihet` (fid, iid, value) and `{out}.{n_samples}.{window}.ldsc`
(chr, pos, M, ldsc) for `gstats` (python/janusx/script/gstats.py; its PDFs and `.gstats.log` are not written).
Only PLINK BED input, the additive model, the -lmm / -fvlmm scans and the GBLUP branch of `-BLUP`
(python/janusx/gs/blup.py:72-163 routes n <= BLUP_SMALL_N there; `gblup_reml_npy_grm` call of
python/janusx/gs/workflow.py:9122) are built; VCF/HMP readers, PCs (-q), plots, the history DB, the
other GS model families are out of scope; `-rrBLUP` runs the exact marker-space route (`rrblup_exact_snp_packed`, REML
lambda from the spectrum) up to 15 000 kept markers and the PCG route (`rrblup_pcg_bed`, HE / manual / subsample-REML
lambda) beyond, `-rr-solver exact|fast|pcg` forces one (fast = exact sample-space route for n_train <= 10 000).
"""
from __future__ import annotations

import argparse
import contextlib
import math
import os
import sys
import time
import types

import numpy as np


SPLMM_APPROX_RHAT_MARKERS = 1000      # python/janusx/assoc/workflow_model_packed.py:99


def _read_table(path):
    """Tab/space delimited table with a header; first column = sample id. -> (ids, names, values float with NaN)."""
    with open(path) as fh:
        header = fh.readline().rstrip("\n").replace(",", "\t").split()
        ids, rows = [], []
        for line in fh:
            parts = line.rstrip("\n").replace(",", "\t").split()
            if not parts:
                continue
            ids.append(parts[0])
            vals = []
            for v in parts[1:]:
                try:
                    vals.append(float(v))
                except ValueError:
                    vals.append(float("nan"))
            rows.append(vals)
    width = max(len(r) for r in rows) if rows else 0
    arr = np.full((len(rows), width), np.nan)
    for i, r in enumerate(rows):
        arr[i, :len(r)] = r
    names = header[1:] if len(header) == width + 1 else [f"trait{i}" for i in range(width)]
    return ids, names, arr


def _select_traits(names, specs):
    if not specs:
        return list(range(len(names)))
    out = []
    for spec in specs:
        for tok in str(spec).split(","):
            tok = tok.strip()
            if ":" in tok and all(t.isdigit() for t in tok.split(":")):
                a, b = [int(t) for t in tok.split(":")]
                out.extend(range(a, b + 1))
            elif tok.isdigit():
                out.append(int(tok))
            elif tok in names:
                out.append(names.index(tok))
            else:
                raise SystemExit(f"unknown trait selector '{tok}'")
    return out


def _load_grm(path, fam_ids):
    k = np.load(path)
    id_path = path + ".id"
    if os.path.exists(id_path):
        ids = [ln.split()[0] for ln in open(id_path) if ln.strip()]
        if ids != list(fam_ids):
            pos = {s: i for i, s in enumerate(ids)}
            try:
                order = np.array([pos[s] for s in fam_ids])
            except KeyError as e:
                raise SystemExit(f"GRM id file lacks sample {e}") from None
            k = k[np.ix_(order, order)]
    if k.shape != (len(fam_ids), len(fam_ids)):
        raise SystemExit(f"GRM shape {k.shape} does not match {len(fam_ids)} samples")
    return np.ascontiguousarray(k, dtype=np.float32)


def _resolve_out(args, src):
    """Output prefix as the reference resolves it (python/janusx/assoc/workflow.py:6907-6921, script/_common/cli_args.py:727-760):
    -o PREFIX or DIR/PREFIX (an existing directory or a trailing separator: the input's basename inside it), -prefix NAME names
    the files inside -o DIR; nothing given: the input's basename in the current directory."""
    base = os.path.basename(src[:-4] if src.lower().endswith((".bed", ".bim", ".fam", ".npy")) else src)
    o, pfx = getattr(args, "out", None), getattr(args, "prefix", None)
    if pfx:
        res = os.path.join(o or ".", pfx)
    elif o is None:
        res = base
    elif o.endswith(os.sep) or os.path.isdir(o):
        res = os.path.join(o, base)
    else:
        res = o
    parent = os.path.dirname(res)
    if parent:
        os.makedirs(parent, exist_ok=True)
    return res


def _dist_setup():
    """Under a launcher (`python -m torch.distributed.run --nproc-per-node N -m janusx_amd gwas ...`: WORLD_SIZE > 1) bind this
    process to its GPU, join the process group (backend JXGPU_DIST_BACKEND, default "nccl" = RCCL over xGMI; "gloo" lets several
    ranks share one GPU in the functional tests) and switch the rank-aware pipeline on: SNP-sharded GRM + one reduction, the
    eigenvectors shared out over the ranks, SNP-sharded scan, rows gathered in BED order.  Rank 0 alone prints
    and writes.  -> (rank, world); (0, 1) without a launcher."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1
    import torch
    import torch.distributed as dist
    from . import pipeline as pl
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("JXGPU_DIST_BACKEND", "nccl")
    ndev = max(1, torch.cuda.device_count())
    if backend == "nccl" and local >= ndev:
        raise SystemExit(f"rank {rank}: local rank {local} has no GPU of its own ({ndev} visible); one process per GPU")
    torch.cuda.set_device(local % ndev)
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local % ndev))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    pl.init_distributed()
    if rank != 0:
        sys.stdout = open(os.devnull, "w")      # one voice: rank 0 reports
    return rank, world


def _check_king_args(args):
    """`jx grm -bfile PREFIX -king [THRESHOLD]`: the combinations that are refused, before any file or device is touched."""
    for flag, on in (("-sparse", args.sparse is not None), ("-grm", args.grm is not None), ("-txt", bool(getattr(args, "txt", False)))):
        if on:
            raise SystemExit(f"grm: -king cannot be combined with {flag}")
    if not args.bfile:
        raise SystemExit("grm: -king needs -bfile PREFIX")
    if not np.isfinite(float(args.king)):
        raise SystemExit("grm: KING kinship_threshold must be finite")


def _cmd_grm_king(args):
    """KING robust kinship of a PLINK prefix (an extension: the reference has the function `king_unrelated_set_from_bed`,
    src/math/KING.rs:794-824, and no command): related pairs, the unrelated set and the removed samples, filtered by this
    command's -maf / -geno / -snps-only with het threshold 0."""
    _check_king_args(args)
    rank, _world = _dist_setup()
    if rank != 0:                                             # one GPU does the work
        return 0
    from . import janusx as jxrs
    from .bed import read_fam_ids
    src = jxrs._bed_prefix(args.bfile)
    out = _resolve_out(args, src)
    t0 = time.perf_counter()
    try:
        kept, removed, pairs, n_sites, n = jxrs._king_from_bed(src, args.maf, args.geno, 0.0, bool(getattr(args, "snps_only", False)),
                                                               float(args.king))
    except (RuntimeError, ValueError) as e:
        raise SystemExit(f"grm: {e}") from None
    ids = read_fam_ids(src)
    if len(ids) != n:
        raise SystemExit(f"grm: {src}.fam lists {len(ids)} samples, the payload has {n}")
    paths = jxrs.write_king_tables(out, ids, n_sites, pairs, kept, removed)
    print(f"KING kinship >= {float(args.king):g}: n={n} sites={n_sites} edges={int(pairs[0].shape[0])} kept={int(kept.shape[0])} "
          f"removed={int(removed.shape[0])} ({time.perf_counter() - t0:.2f}s)")
    for path in paths:
        print(f"  {path}")
    return 0


def cmd_grm(args):
    from . import janusx as jxrs
    from .bed import read_fam_ids
    if args.grm is None and not args.bfile:
        raise SystemExit("grm needs -bfile PREFIX (or -grm FILE.npy -sparse [cutoff])")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and args.grm is not None:
        raise SystemExit("thresholding an existing dense GRM runs on one GPU: start it without the launcher")
    if getattr(args, "king", None) is not None:
        return _cmd_grm_king(args)
    out = _resolve_out(args, args.bfile or args.grm)
    t0 = time.perf_counter()
    if args.grm is not None:
        # python/janusx/script/grm.py:1806-1868, 1896: an existing dense GRM (`.npy` + sibling `.id`) thresholded into `.spgrm`
        if args.sparse is None:
            raise SystemExit("-grm FILE.npy must be used with -sparse [cutoff]")
        if not os.path.exists(args.grm + ".id"):
            raise SystemExit(f"{args.grm}.id not found (sample ids of the dense GRM)")
        path, n, nnz = jxrs.spgrm_dense_npy_to_jxgrm(args.grm, out, float(args.sparse))
        ids_in = open(args.grm + ".id").read().split()
        if len(ids_in) != n:
            raise SystemExit(f"{args.grm}.id lists {len(ids_in)} samples, the matrix has {n}")
        with open(path + ".id", "w") as fh:
            for sid in ids_in:
                fh.write(f"{sid}\n")
        print(f"Sparse GRM from {args.grm}: n={n} nnz={nnz} cutoff={args.sparse} -> {path} "
              f"({time.perf_counter() - t0:.2f}s)")
        return 0
    if args.sparse is not None:
        # python/janusx/script/grm.py:1574-1675 (`-sparse [cutoff]`): thresholded lower-triangle CSC `.spgrm` + `.id`; under
        # the launcher the row panels of the matrix are dealt over the ranks (janusx._spgrm_packed)
        rank, world = _dist_setup()
        path, n, nnz = jxrs.spgrm_bed_to_jxgrm(args.bfile, out_prefix=out, method=args.method,
                                               threshold=float(args.sparse), maf_threshold=args.maf,
                                               max_missing_rate=args.geno, het_threshold=0.0,
                                               snps_only=bool(getattr(args, "snps_only", False)))
        if rank == 0:
            with open(path + ".id", "w") as fh:
                for sid in read_fam_ids(args.bfile):
                    fh.write(f"{sid}\n")
        print(f"Sparse GRM method {args.method}: n={n} nnz={nnz} cutoff={args.sparse} -> {path} "
              f"({time.perf_counter() - t0:.2f}s)")
        return 0
    rank, world = _dist_setup()
    if world > 1:
        # one process per GPU: every rank accumulates its share of the kept SNPs, one reduction over xGMI (pipeline.build_grm)
        import torch
        from . import pipeline as pl
        from .bed import snps_only_mask, stage_bed_payload
        packed_t, n, bim = stage_bed_payload(args.bfile, None)
        if getattr(args, "snps_only", False):
            packed_t = packed_t[torch.from_numpy(np.nonzero(snps_only_mask(bim))[0]).to(packed_t.device)]
        k_t, eff, _ = pl.build_grm(packed_t, n, args.method, args.maf, args.geno)
        if rank != 0:
            return 0
        k = k_t.cpu().numpy()
    else:
        k, eff, n = jxrs.grm_stream_bed_f32(args.bfile, method=args.method, maf_threshold=args.maf,
                                            max_missing_rate=args.geno, het_threshold=0.0,
                                            snps_only=bool(getattr(args, "snps_only", False)))
    tag = "cGRM" if args.method == 1 else "sGRM"
    if getattr(args, "txt", False):             # python/janusx/script/grm.py:2684-2690
        path = f"{out}.{tag}.txt"
        tmp = f"{path}.tmp.{os.getpid()}"
        np.savetxt(tmp, k, fmt="%.6f")
    else:
        path = f"{out}.{tag}.npy"
        tmp = f"{path}.tmp.{os.getpid()}"
        with open(tmp, "wb") as fh:
            np.lib.format.write_array(fh, k, version=(1, 0))
    os.replace(tmp, path)
    with open(path + ".id", "w") as fh:
        for sid in read_fam_ids(args.bfile):
            fh.write(f"{sid}\n")
    print(f"GRM method {args.method}: n={n} eff_m={eff} -> {path} ({time.perf_counter() - t0:.2f}s)")
    return 0


def build_cv_splits(n_samples, n_splits, seed=42):
    """`build_cv_splits` (python/janusx/gs/workflow.py:3950-3980) over the `KFold` of python/janusx/pyBLUP/kfold.py:28-88:
    one permutation of arange(n) from numpy's default_rng(seed), cut into n_splits runs whose sizes differ by at most one
    (the first n % k folds are the longer ones); each item is (test_idx, train_idx), train in ascending order."""
    n, k = int(n_samples), int(n_splits)
    if n < 2:
        raise ValueError(f"CV requires at least 2 samples, got {n}.")
    if k < 2:
        raise ValueError(f"CV folds must be >=2, got {k}.")
    if k > n:
        raise ValueError(f"CV folds ({k}) cannot exceed sample size ({n}).")
    idx = np.asarray(np.random.default_rng(int(seed)).permutation(np.arange(n, dtype=np.int64)), dtype=np.int64)
    sizes = np.full(k, n // k, dtype=np.int64)
    sizes[: n % k] += 1
    out, cur = [], 0
    for fs in sizes:
        te = idx[cur:cur + int(fs)]
        cur += int(fs)
        mask = np.zeros(n, dtype=bool)
        mask[te] = True
        out.append((te, np.nonzero(~mask)[0].astype(np.int64)))
    return out


def cv_fold_metrics(y_true, y_pred):
    """Per-fold metrics of the reference's GS summary (python/janusx/gs/workflow.py:880-930): Pearson r, Spearman rho,
    R2 = 1 - SS_res / SS_tot of the held-out fold."""
    from scipy.stats import pearsonr, spearmanr
    yt, yp = np.asarray(y_true, dtype=np.float64), np.asarray(y_pred, dtype=np.float64)
    ss_res = float(np.sum((yt - yp) ** 2))
    ss_tot = float(np.sum((yt - float(np.mean(yt))) ** 2))
    r2 = 1.0 - ss_res / ss_tot if ss_tot > 0.0 else 0.0
    return float(pearsonr(yt, yp).statistic), float(spearmanr(yt, yp).statistic), r2


def _parse_qcov_dim(qcov_opt) -> int:
    """`_parse_qcov_dim` (python/janusx/assoc/workflow.py:1813-1828): -q takes a PC count, not a file."""
    s = str(qcov_opt if qcov_opt is not None else "").strip()
    if s == "":
        raise SystemExit("Invalid -q/--qcov: empty value. Use an integer PC dimension (>=0).")
    try:
        q = int(s)
    except ValueError:
        raise SystemExit("External Q matrix via -q/--qcov is no longer supported. Use -c <file> for external covariates and "
                         "-q <int> for the PC dimension.")
    if q < 0:
        raise SystemExit(f"Invalid -q/--qcov: {q}. Q/PC dimension must be >= 0.")
    return q


def _parse_cov_site_token(token):
    """`_parse_cov_site_token` (python/janusx/assoc/workflow.py:1742-1776): chr:pos or chr:start:end with start = end."""
    parts = [p.strip() for p in str(token).strip().replace("\uff1a", ":").split(":")]
    if len(parts) not in (2, 3) or parts[0] == "":
        return None
    try:
        start = int(float(parts[1]))
    except Exception:
        return None
    if start <= 0:
        raise SystemExit(f"Invalid site position in --cov: {token}")
    if len(parts) == 3:
        try:
            end = int(float(parts[2]))
        except Exception:
            return None
        if end <= 0:
            raise SystemExit(f"Invalid site position in --cov: {token}")
        if end != start:
            raise SystemExit(f"--cov site token must specify a single site (start=end), got: {token}")
    return parts[0], start


def _canon_site_key(chrom, pos):
    c = str(chrom).strip().lower()
    return (c[3:] if c.startswith("chr") else c), int(pos)


def _warm_start_mode(args):
    """'chain' | 'none' for `jx gwas -lmm`: the flag, else the reference's rule (chain unless JX_LMM_UNIFIED_NO_WARM_START)."""
    from .stats import env_truthy
    if getattr(args, "warm_start", None) is not None:
        return args.warm_start
    return "none" if env_truthy("JX_LMM_UNIFIED_NO_WARM_START") else "chain"


def _parse_lm2_covariate_selector(value, label="-lm2/--lm2"):
    """`_parse_lm2_covariate_selector` (python/janusx/assoc/workflow.py:497-553): 0-based column selectors `0`, `0:3` (both ends
    included, descending allowed), `:2`, `0,3`; duplicates are dropped in first-seen order; a bare flag selects nothing."""
    raw = str(value).strip() if value is not None else ""
    if raw in ("", "__SELF__"):
        return []
    picks = []

    def push(idx0):
        if idx0 < 0:
            raise ValueError(f"{label}: covariate column indices must be >= 0, got {idx0}.")
        if idx0 not in picks:
            picks.append(idx0)

    def is_int(tok):
        return tok.lstrip("+-").isdigit()

    for token in [t.strip() for t in raw.split(",") if t.strip() != ""]:
        if ":" in token:
            left, right = (t.strip() for t in token.split(":", 1))
            if left == "" and right == "":
                raise ValueError(f"{label}: invalid empty covariate range '{token}'.")
            if left != "" and not is_int(left):
                raise ValueError(f"{label}: invalid covariate range start '{left}'.")
            start = 0 if left == "" else int(left)
            if right == "":
                raise ValueError(f"{label}: open-ended covariate range '{token}' is not supported; provide an explicit end.")
            if not is_int(right):
                raise ValueError(f"{label}: invalid covariate range end '{right}'.")
            end = int(right)
            step = 1 if end >= start else -1
            for idx in range(start, end + step, step):
                push(idx)
            continue
        if not is_int(token):
            raise ValueError(f"{label}: invalid covariate selector '{token}'. Use 0-based indices/ranges like 0, 0:3, :2, 0,3.")
        push(int(token))
    return picks


def _resolve_lm2_covariate_indices(cov_all, selector_zero_based, label="-lm2/--lm2"):
    """`_resolve_lm2_covariate_indices` (python/janusx/assoc/workflow.py:556-575): the selection against the merged -c table."""
    arr = np.asarray(cov_all)
    if arr.ndim != 2:
        raise ValueError("LM2 requires a 2D merged covariate matrix.")
    ncov = int(arr.shape[1])
    if ncov <= 0:
        raise ValueError("LM2 requires at least one covariate column from -c.")
    bad = [int(i) for i in selector_zero_based if int(i) < 0 or int(i) >= ncov]
    if bad:
        raise ValueError(f"{label}: covariate column index out of range: {bad[0]}. valid=[0..{ncov - 1}]")
    return np.asarray(selector_zero_based, dtype=np.int64)


def _run_lm_models(packed_t, n_fam, keep_idx, y, x, cov_rows, lm2_idx, run_lm, args, bim, out, name):
    """`-lm` and `-lm2` of one trait on one panel of its samples: the QC of the other models (-maf, -geno, -het), the plain LM
    scan (`pipeline.scan_rows_lm`, the table the LRT fallback of -lmm writes) and / or the interaction scan
    (`pipeline.scan_rows_lm2`); `af` = ALT frequency, `miss` = the count of missing samples."""
    from . import pipeline as pl
    from . import stats as st
    from .tsv import write_assoc_tsv_counts, write_lm2_tsv
    n = len(keep_idx)
    # a panel of its own, released on return: with -lmm / -lmm2 / -fvlmm in the same run `run_trait` re-tiles the payload once
    # more for the same samples (one repack pass per trait; the two images are never resident together)
    panel = pl.Panel(packed_t, n_fam, keep_idx)
    counts = panel.counts()
    keep, af, _miss = st.gwas_scan_row_stats(counts, n, args.maf, args.geno, args.het)
    rows = np.nonzero(keep)[0]
    meta = bim.columns(rows)
    miss_cnt = counts[rows, 0]
    if run_lm:
        t1 = time.perf_counter()
        path = f"{out}.{name}.lm.tsv"
        stats = pl.scan_rows_lm(panel, rows, af[rows], x, y)
        write_assoc_tsv_counts(path, *meta, af[rows], miss_cnt.astype(np.float32), stats[:, :3].cpu().numpy())
        print(f"[{name}] -lm: n={n} snps={len(rows)} -> {path} ({time.perf_counter() - t1:.2f}s)")
    if lm2_idx is not None:
        t1 = time.perf_counter()
        path = f"{out}.{name}.lm2.tsv"
        stats = pl.scan_rows_lm2(panel, rows, af[rows], x, cov_rows[:, lm2_idx], y)
        write_lm2_tsv(path, *meta, af[rows], miss_cnt, stats.cpu().numpy(), [int(i) for i in lm2_idx])
        print(f"[{name}] -lm2: n={n} snps={len(rows)} interactions={','.join(str(int(i)) for i in lm2_idx)} -> {path} "
              f"({time.perf_counter() - t1:.2f}s)")


def _parse_farmcpu_args(args):
    """The FarmCPU options of `jx gwas` (python/janusx/assoc/workflow.py:6727-6790) -> dict for `farmcpu.run_raw`."""
    if int(args.farmcpu_iter) < 1:
        raise SystemExit("--farmcpu-iter must be >= 1")
    thr = args.farmcpu_threshold
    if thr is not None and not (math.isfinite(thr) and thr > 0.0):
        raise SystemExit("--farmcpu-threshold must be finite and > 0")
    qb = str(args.farmcpu_qtn_bound).strip().lower()
    if qb in ("auto", ""):
        bound = None
    else:
        try:
            bound = int(qb)
        except ValueError:
            raise SystemExit(f"--farmcpu-qtn-bound {args.farmcpu_qtn_bound}: expected auto or an integer >= 1")
        if bound < 1:
            raise SystemExit("--farmcpu-qtn-bound must be >= 1")
    if int(args.farmcpu_nbin) < 1:
        raise SystemExit("--farmcpu-nbin must be >= 1")
    try:
        szbin = [float(t) for t in str(args.farmcpu_bin_size).split(",") if t.strip()]
    except ValueError:
        raise SystemExit(f"--farmcpu-bin-size {args.farmcpu_bin_size}: expected comma-separated numbers")
    if not szbin or any(not (math.isfinite(v) and v > 0.0) for v in szbin):
        raise SystemExit("--farmcpu-bin-size: every bin size must be finite and > 0")
    return {"threshold": thr, "max_iter": int(args.farmcpu_iter), "qtn_bound": bound, "nbin": int(args.farmcpu_nbin),
            "szbin": szbin}


def _run_farmcpu(packed_t, n_fam, keep_idx, y, x, farm, args, bim, out, name):
    """`-farmcpu` of one trait on a panel of its samples: the QC of the other models, then `farmcpu.run_raw` with the design
    [1 | Q | C] as the base; `af` = ALT frequency, `miss` = the count of missing samples."""
    from . import farmcpu as fc
    from . import pipeline as pl
    from . import stats as st
    t1 = time.perf_counter()
    n = len(keep_idx)
    panel = pl.Panel(packed_t, n_fam, keep_idx)
    keep, af, _miss = st.gwas_scan_row_stats(panel.counts(), n, args.maf, args.geno, args.het)
    rows = np.nonzero(keep)[0]
    if len(rows) == 0:
        print(f"[{name}] -farmcpu: no SNP passes the filters, skipped")
        return
    chrom, pos, snp, a0, a1 = bim.columns(rows)
    thr = farm["threshold"] if farm["threshold"] is not None else 1.0 / len(rows)
    res = fc.run_raw(panel, rows, af[rows], np.zeros(len(rows), dtype=bool), y, x, chrom, pos, thr, farm["max_iter"],
                     farm["qtn_bound"], farm["nbin"], farm["szbin"])
    path = f"{out}.{name}.farmcpu.tsv"
    fc.write_main_tsv(path, chrom, pos, snp, a0, a1, af[rows], res.miss, res.stats)
    note = ""
    if res.qtn:
        fc.write_qtn_tsv(f"{out}.{name}.farmcpu.qtn", res.qtn, chrom, pos, snp, a0, a1, af[rows], res.miss, res.stats, rows)
        note = f", {out}.{name}.farmcpu.qtn"
    print(f"[{name}] -farmcpu: n={n} snps={len(rows)} iterations={len(res.trace)} qtn={len(res.qtn)} -> {path}{note} "
          f"({time.perf_counter() - t1:.2f}s)")


def group_traits_by_samples(traits, samples_of):
    """Traits (column indices, in selection order) grouped by their sample set: -> [(keep_idx, [trait, ...])], the groups in the
    order of their first trait, the traits of a group in selection order.  `samples_of(trait)` -> int64 FAM positions."""
    groups, where = [], {}
    for ti in traits:
        keep_idx = np.asarray(samples_of(ti), dtype=np.int64)
        key = keep_idx.tobytes()
        if key not in where:
            where[key] = len(groups)
            groups.append((keep_idx, []))
        groups[where[key]][1].append(ti)
    return groups


def _run_lm_trait_level(packed_t, n_fam, traits, names, samples_of, design_of, y_of, args, bim, out, pmax):
    """`jx gwas -lm -trait-level`: the traits grouped by sample mask; per group one panel, one QC pass (-maf, -geno, -het), one
    design and one multi-trait scan (`janusx._lm_traits_group`; a group of one trait takes the single-trait scan), all into the
    combined table {out}.lm.tsv with `miss` as the count of missing samples."""
    from . import janusx as jxrs
    from . import pipeline as pl
    from . import stats as st
    from .tsv import TraitTableWriter, resolve_snp_name, trait_site_prefixes
    t0 = time.perf_counter()
    path = f"{out}.lm.tsv"
    writer = TraitTableWriter(path)
    done = 0
    try:
        for keep_idx, members in group_traits_by_samples(traits, samples_of):
            n = len(keep_idx)
            label = ",".join(names[ti] for ti in members[:3]) + ("" if len(members) <= 3 else f",... ({len(members)} traits)")
            if n < 10:
                print(f"[{label}] only {n} phenotyped samples, skipped")
                continue
            t1 = time.perf_counter()
            panel = pl.Panel(packed_t, n_fam, keep_idx)
            counts = panel.counts()
            keep, af, _miss = st.gwas_scan_row_stats(counts, n, args.maf, args.geno, args.het)
            rows = np.nonzero(keep)[0]
            chrom, pos, snp, a0, a1 = bim.columns(rows)
            prefixes = trait_site_prefixes(chrom, pos, [resolve_snp_name(*spc) for spc in zip(snp, chrom, pos)], a0, a1, af[rows],
                                           counts[rows, 0].astype(np.float32), as_rate=False)
            y = np.stack([y_of(keep_idx, ti) for ti in members])
            jxrs._lm_traits_group(writer, panel, rows, np.zeros(len(rows), dtype=bool), af[rows], design_of(keep_idx), y,
                                  [names[ti] for ti in members], prefixes, pmax)
            done += len(members)
            print(f"[{label}] -lm -trait-level: n={n} snps={len(rows)} traits={len(members)} ({time.perf_counter() - t1:.2f}s)")
            del panel
    except BaseException:
        writer.abort()
        raise
    lines = writer.close()
    print(f"-lm -trait-level: {done} traits, {lines} rows -> {path} ({time.perf_counter() - t0:.2f}s)")


def _run_lmm_trait_level(packed_t, n_fam, k, traits, names, samples_of, design_of, y_of, args, bim, out, pmax):
    """`jx gwas -lmm -trait-level-lmm`: the traits grouped by sample mask; per group ONE eigendecomposition, ONE rotation of the
    design and of every SNP block for all its traits (`pipeline.run_traits_lmm`; a group of one trait takes the same code), all
    into the combined table {out}.lmm.tsv: per trait the lines of its single-trait `.lmm.tsv` (`miss` as a rate) followed by the
    phenotype column.  Unless -force-model, a group in which the null likelihood-ratio test sends any trait to the LM is left to
    the trait-by-trait route.  -> the traits written here."""
    from . import pipeline as pl
    from .tsv import TraitTableWriter, assoc_trait_stats, resolve_snp_name, trait_site_prefixes
    t0 = time.perf_counter()
    path = f"{out}.lmm.tsv"
    writer = TraitTableWriter(path)
    chain = None
    if _warm_start_mode(args) == "chain":
        chain = (max(1, int(args.chunksize)), max(1, int(args.warm_chain_pieces)))
    done = set()
    try:
        for keep_idx, members in group_traits_by_samples(traits, samples_of):
            n = len(keep_idx)
            label = ",".join(names[ti] for ti in members[:3]) + ("" if len(members) <= 3 else f",... ({len(members)} traits)")
            if n < 10:
                continue                 # the trait-by-trait loop reports it
            t1 = time.perf_counter()
            y = np.stack([y_of(keep_idx, ti) for ti in members])
            res = pl.run_traits_lmm(packed_t, n_fam, k, keep_idx, y, design_of(keep_idx), args.maf, args.geno, args.het,
                                    force_model=bool(args.force_model), warm_chain=chain)
            if res.switch is not None:
                _sw, stat, pv = res.null_lrt[res.switch]
                print(f"[{label}] Warning: -trait-level-lmm: trait {names[members[res.switch]]} would switch to LM (null LRT "
                      f"stat={stat:.4g}, p={pv:.4g} >= 0.05); this group goes trait by trait")
                continue
            rows = np.nonzero(res.keep)[0]
            chrom, pos, snp, a0, a1 = bim.columns(rows)
            prefixes = trait_site_prefixes(chrom, pos, [resolve_snp_name(*spc) for spc in zip(snp, chrom, pos)], a0, a1, res.af,
                                           res.miss, as_rate=True)
            for pos_t, ti in enumerate(members):
                st4 = assoc_trait_stats(res.stats[pos_t])
                if pmax is None:
                    writer.put(prefixes, st4, names[ti])
                else:
                    hit = np.nonzero(st4[:, 3] <= float(pmax))[0]
                    writer.put(prefixes, st4[hit], names[ti], hit)
                done.add(ti)
            nulls = " ".join(f"{names[ti]}:lambda0={nf.lbd:.5g},pve={nf.pve:.4f}" for ti, nf in zip(members[:3], res.nulls))
            print(f"[{label}] -lmm -trait-level-lmm: n={n} snps={len(rows)} traits={len(members)} {nulls} "
                  f"({time.perf_counter() - t1:.2f}s)")
    except BaseException:
        writer.abort()
        raise
    lines = writer.close()
    print(f"-lmm -trait-level-lmm: {len(done)} traits, {lines} rows -> {path} ({time.perf_counter() - t0:.2f}s)")
    return done


def _load_cov_items(cov_items, fam, bim, packed_t, n_fam):
    """The -c items of a run joined on the samples they share -> (cv (samples, columns) f64, {sample id: row}), or (None, {})
    when no item gave columns.  An item is a covariate table or a SNP site `chr:pos` (`chr:start:end` with start = end) whose
    additive genotype -- missing calls at the site's mean over all genotyped samples -- becomes a covariate (conditional analysis;
    `_load_covariates_for_models` / `_load_site_covariates`, python/janusx/assoc/workflow.py:1742-1789, 1979-2145)."""
    cv, cpos = None, {}
    if cov_items:
        parts = []
        for item in cov_items:
            site = _parse_cov_site_token(item)
            if site is None:
                if not os.path.isfile(item):
                    print(f"Covariate file not found: {item}; skipped.")
                    continue
                cids_i, _, cv_i = _read_table(item)
                parts.append((list(cids_i), np.asarray(cv_i, dtype=np.float64).reshape(len(cids_i), -1)))
            else:
                key = _canon_site_key(*site)
                hit = next((j for j in range(len(bim.chrom)) if _canon_site_key(bim.chrom[j], bim.pos[j]) == key), None)
                if hit is None:
                    raise SystemExit(f"Some --cov SNP site(s) were not found in genotype: {site[0]}:{site[1]}")
                row = packed_t[hit].cpu().numpy()
                codes = ((row[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)[:n_fam]
                gv = np.array([0.0, np.nan, 1.0, 2.0])[codes]
                gv[np.isnan(gv)] = float(np.nanmean(gv)) if np.isfinite(gv).any() else 0.0
                parts.append((list(fam), gv.reshape(-1, 1)))
        if parts:
            common = set(parts[0][0])
            for ids_i, _m in parts[1:]:
                common &= set(ids_i)
            cids = [sid for sid in fam if sid in common]
            if not cids:
                raise SystemExit("No overlapping samples between genotype and covariates.")
            cols = []
            for ids_i, m_i in parts:
                ix = {sid: i for i, sid in enumerate(ids_i)}
                cols.append(m_i[[ix[sid] for sid in cids]])
            cv = np.concatenate(cols, axis=1)
            cpos = {s: i for i, s in enumerate(cids)}
    return cv, cpos


def cmd_gwas(args):
    import torch
    from . import janusx as jxrs
    from . import pipeline as pl
    from .bed import read_bed_payload, read_fam_ids
    from .tsv import AsyncAssocTsvWriter, write_assoc_tsv
    # SparseLMM flags of the reference (python/janusx/assoc/workflow.py:6689-6725, 6992-7017): -splmm-exact = exact g'Pg scan,
    # raw REML null objective, result stem "splmm2"; -splmm = fastGWA fixed-Vp null objective + residualised GRAMMAR-gamma
    # denominator from 1000 sampled markers, stem "splmm" (a trait with fewer kept markers than that falls back to the exact
    # scan, workflow_model_packed.py:8087-8107)
    sp_stems = []
    if getattr(args, "splmm_exact", None) is not None:
        sp_stems.append("splmm2")
    if args.splmm is not None:
        sp_stems.append("splmm")
        if getattr(args, "splmm_exact", None) is not None and float(args.splmm_exact) != float(args.splmm):
            raise SystemExit("-splmm and -splmm-exact in one run must use the same sparse-GRM cut-off")
    if args.splmm is None and sp_stems:
        args.splmm = float(args.splmm_exact)
    lm2_flag = getattr(args, "lm2", None)
    run_farmcpu = bool(getattr(args, "farmcpu", False))
    if getattr(args, "frgwas", False) or getattr(args, "algwas", False):
        raise SystemExit("-frgwas / -algwas (the unified FarmCPU routes) are not built; -farmcpu runs the classic route")
    if not (getattr(args, "lm", False) or lm2_flag is not None or args.lmm or args.fvlmm or args.lmm2 or args.splmm is not None
            or run_farmcpu):
        raise SystemExit("select at least one model: -lm, -lm2, -lmm, -lmm2, -fvlmm, -splmm and/or -splmm-exact")
    farm = _parse_farmcpu_args(args) if run_farmcpu else None
    try:
        lm2_sel = _parse_lm2_covariate_selector(lm2_flag)
    except ValueError as e:
        raise SystemExit(str(e))
    trait_level = bool(getattr(args, "trait_level", False))
    trait_pmax = getattr(args, "trait_pmax", None)
    trait_lmm = bool(getattr(args, "trait_level_lmm", False))
    if trait_pmax is not None and not (trait_level or trait_lmm):
        raise SystemExit("-trait-pmax belongs to -trait-level")
    if run_farmcpu and (trait_level or trait_lmm):
        raise SystemExit("-farmcpu goes trait by trait: it does not combine with -trait-level / -trait-level-lmm")
    if trait_level:
        # the reference's conditions (python/janusx/assoc/workflow_model_packed.py:5046-5064), before anything is loaded
        if not getattr(args, "lm", False):
            raise SystemExit("-trait-level: the LM trait-level route requires -lm (the trait-level route of -lmm is -trait-level-lmm).")
        if trait_pmax is not None and not (0.0 <= float(trait_pmax) <= 1.0):
            raise SystemExit("-trait-pmax must be within [0, 1]")
        if len(_select_traits(_read_table(args.pheno)[1], args.ncol)) <= 1:
            raise SystemExit("LM trait-level route requires at least 2 traits.")
    if trait_lmm:
        if not args.lmm:
            raise SystemExit("-trait-level-lmm: the LMM trait-level route requires -lmm.")
        if trait_pmax is not None and not (0.0 <= float(trait_pmax) <= 1.0):
            raise SystemExit("-trait-pmax must be within [0, 1]")
        if len(_select_traits(_read_table(args.pheno)[1], args.ncol)) <= 1:
            raise SystemExit("LMM trait-level route requires at least 2 traits.")
    rank, world = _dist_setup()
    # the payload goes to HBM in windows (bed.stage_bed_payload: `mmap_window_mb` of the reference's BED routes); nothing
    # below holds a host copy of it
    from .bed import stage_bed_payload
    packed_t, n_fam, bim = stage_bed_payload(args.bfile, getattr(args, "mmap_window_mb", None))
    if getattr(args, "snps_only", False):
        # -snps-only: sites whose two alleles are not single A/C/G/T leave the run altogether -- GRM, QC and scan
        # (`snps_only` of the reference's BED routes, src/io/gfreader.rs:7013-7019)
        from .bed import snps_only_mask
        mask = snps_only_mask(bim)
        if not mask.all():
            sel = np.nonzero(mask)[0]
            packed_t = packed_t[torch.from_numpy(sel).to(packed_t.device)]
            bim = bim.take(sel)
            print(f"-snps-only: {len(sel)} of {len(mask)} sites kept")
    packed = packed_t
    fam = read_fam_ids(args.bfile)
    ids, names, ph = _read_table(args.pheno)
    pos = {s: i for i, s in enumerate(ids)}
    # -c may be repeated; an item is a covariate table or a SNP site `chr:pos` (`chr:start:end` with start = end) whose additive
    # genotype -- missing calls at the site's mean over all genotyped samples -- becomes a covariate (conditional analysis;
    # `_load_covariates_for_models` / `_load_site_covariates`, python/janusx/assoc/workflow.py:1742-1789, 1979-2145).  The
    # columns of all items are joined on the samples they share.
    cov_items = args.cov if isinstance(args.cov, list) else ([args.cov] if args.cov else [])
    cv, cpos = _load_cov_items(cov_items, fam, bim, packed_t, n_fam)
    args.cov = cv is not None
    # -lm2 without -c, or without COVCOL, runs -lm instead (python/janusx/assoc/workflow.py:7969-8001); once, if -lm was given too
    run_lm, lm2_idx = bool(getattr(args, "lm", False)), None
    if lm2_flag is not None:
        if not args.cov:
            print("Warning: LM2 received no external covariates from -c; falling back to LM.")
            run_lm = True
        elif not lm2_sel:
            print("Warning: LM2 received no explicit interaction columns; falling back to LM.")
            run_lm = True
        else:
            from .lm2 import LM2_MAX_INTERACTIONS
            try:
                lm2_idx = _resolve_lm2_covariate_indices(cv, lm2_sel)
            except ValueError as e:
                raise SystemExit(str(e))
            if len(lm2_idx) > LM2_MAX_INTERACTIONS:
                raise SystemExit(f"-lm2/--lm2: at most {LM2_MAX_INTERACTIONS} interaction columns in this build, got {len(lm2_idx)}")
    if (run_lm or lm2_idx is not None) and world > 1:
        print("-lm / -lm2: computed on rank 0 alone")
    if run_farmcpu and world > 1:
        print("-farmcpu: computed on rank 0 alone")
    traits = _select_traits(names, args.ncol)
    out = _resolve_out(args, args.bfile)
    dev = packed_t.device
    t0 = time.perf_counter()
    dense_models = args.lmm or args.fvlmm or args.lmm2
    k = None
    if dense_models and str(args.grm).lower().endswith((".spgrm", ".jxgrm")):
        raise SystemExit("-k FILE.spgrm is a sparse GRM: it serves -splmm only; -lmm / -lmm2 / -fvlmm need a dense GRM "
                         "(-k 1 | 2 | FILE.npy)")
    if dense_models and args.grm in ("1", "2"):
        k, eff, _ = pl.build_grm(packed_t, n_fam, int(args.grm), args.maf, args.geno)
        print(f"GRM method {args.grm}: eff_m={eff} ({time.perf_counter() - t0:.2f}s)")
    elif dense_models:
        k = torch.from_numpy(_load_grm(args.grm, fam)).to(dev)    # every rank reads the same file
    # -q N: the N leading principal components of the whole-cohort GRM as fixed-effect columns beside the intercept
    # (`load_or_build_q_with_cache` -> `build_pcs_from_grm`, python/janusx/assoc/workflow.py:3389-3422, 3577-3789: the last N
    # columns of the ascending eigendecomposition of the GRM without a ridge, stored as f32; the reference switches to a
    # randomised SVD of the genotypes above 15 000 samples, here the GRM route serves every size)
    qdim = _parse_qcov_dim(getattr(args, "qcov", "0"))
    qmat = None
    if qdim > 0:
        if qdim >= n_fam:
            raise SystemExit(f"Q/PC dimension out of range: {qdim}. valid=[0..{max(0, n_fam - 1)}]")
        kq = k
        if kq is None:
            kq, _eff_q, _ = pl.build_grm(packed_t, n_fam, int(args.grm) if args.grm in ("1", "2") else 1, args.maf, args.geno)
        tq = time.perf_counter()
        _s_all, ut_all = pl.eigh_from_grm(kq, ridge=0.0)
        qmat = ut_all[-qdim:].T.to(torch.float32).cpu().numpy().astype(np.float64)
        del _s_all, ut_all, kq
        print(f"Q matrix: {qdim} principal components of the GRM ({time.perf_counter() - tq:.2f}s)")
    sparse_path = None
    sparse_pos = None
    if args.splmm is not None:
        # SparseLMM, exact mode: thresholded sparse GRM of all genotyped samples once (`.spgrm`, or an existing one given
        # with -grm FILE.spgrm), then per trait the sparse REML null model and the exact g'Pg scan on its samples
        # -spk / --grm-sparse (python/janusx/assoc/workflow.py:6747-6754): 1 | 2 = method of the sparse GRM built here, or the
        # path of a precomputed .spgrm / .jxgrm; -k FILE.spgrm is this build's older way of naming the same file
        spk = str(getattr(args, "grm_sparse", "1") or "1").strip()
        spk_file = spk if spk.lower().endswith((".spgrm", ".jxgrm")) else None
        if spk_file is None and spk not in ("1", "2"):
            raise SystemExit(f"-spk {spk}: expected 1 (centering), 2 (standardization) or a .spgrm / .jxgrm file "
                             "(GCTA / fastGWA .grm.sp inputs are not read by this build)")
        if spk_file is not None or str(args.grm).lower().endswith((".spgrm", ".jxgrm")):
            sparse_path = spk_file if spk_file is not None else args.grm
            # the sparse GRM's own sample order: map by id, like the dense -grm FILE path (_load_grm)
            id_path = sparse_path + ".id"
            if not os.path.exists(id_path):
                raise SystemExit(f"{id_path} not found: a sparse GRM given with -k needs its sample-id file "
                                 "(one id per line, in the order of the matrix)")
            sparse_ids = [ln.split()[0] for ln in open(id_path) if ln.strip()]
            sparse_pos = {sid: i for i, sid in enumerate(sparse_ids)}
            if len(sparse_pos) != len(sparse_ids):
                raise SystemExit(f"{id_path} lists duplicate sample ids")
        else:
            method = int(spk) if spk == "2" else (int(args.grm) if args.grm in ("1", "2") else 1)
            sparse_path, _, nnz = jxrs.spgrm_bed_to_jxgrm(args.bfile, out_prefix=out, method=method,
                                                         threshold=float(args.splmm), maf_threshold=args.maf,
                                                         max_missing_rate=args.geno, het_threshold=0.0,
                                                         snps_only=bool(getattr(args, "snps_only", False)))
            if rank == 0:
                with open(sparse_path + ".id", "w") as fh:
                    for sid in fam:
                        fh.write(f"{sid}\n")
            print(f"Sparse GRM cutoff={args.splmm}: nnz={nnz} -> {sparse_path} ({time.perf_counter() - t0:.2f}s)")
    def trait_samples(ti):
        """FAM positions of the samples of trait `ti`: a finite phenotype and, with -c, finite covariates."""
        rows_ok = []
        for j, sid in enumerate(fam):
            i = pos.get(sid)
            if i is None or not math.isfinite(ph[i, ti]):
                continue
            if args.cov and (sid not in cpos or not np.all(np.isfinite(cv[cpos[sid]]))):
                continue
            rows_ok.append(j)
        return np.array(rows_ok, dtype=np.int64)

    def trait_design(keep_idx):
        x = np.ones((len(keep_idx), 1))
        if qmat is not None:                    # design = [1 | Q | C] (workflow.py:1545-1560)
            x = np.concatenate([x, qmat[keep_idx]], axis=1)
        if args.cov:
            x = np.concatenate([x, np.array([cv[cpos[fam[j]]] for j in keep_idx])], axis=1)
        return x

    if trait_level:
        if lm2_idx is not None or dense_models or args.splmm is not None:
            print("-trait-level: serves -lm; the other models of this run go trait by trait as without it")
        if rank == 0:
            _run_lm_trait_level(packed_t, n_fam, traits, names, trait_samples, trait_design,
                                lambda keep_idx, ti: np.array([ph[pos[fam[j]], ti] for j in keep_idx]), args, bim, out, trait_pmax)
        run_lm = False
    lmm_done = set()      # traits whose -lmm rows went into the combined table of -trait-level-lmm
    if trait_lmm:
        if world > 1:
            print("-trait-level-lmm: one rank only; -lmm goes trait by trait as without it")
        else:
            lmm_done = _run_lmm_trait_level(packed_t, n_fam, k, traits, names, trait_samples, trait_design,
                                            lambda keep_idx, ti: np.array([ph[pos[fam[j]], ti] for j in keep_idx]), args, bim, out,
                                            trait_pmax)
    for ti in traits:
        name = names[ti]
        keep_idx = trait_samples(ti)
        n = len(keep_idx)
        if n < 10:
            print(f"[{name}] only {n} phenotyped samples, skipped")
            continue
        y = np.array([ph[pos[fam[j]], ti] for j in keep_idx])
        x = trait_design(keep_idx)
        if (run_lm or lm2_idx is not None) and rank == 0:
            cov_rows = np.array([cv[cpos[fam[j]]] for j in keep_idx]) if lm2_idx is not None else None
            _run_lm_models(packed_t, n_fam, keep_idx, y, x, cov_rows, lm2_idx, run_lm, args, bim, out, name)
        if run_farmcpu and rank == 0:
            _run_farmcpu(packed_t, n_fam, keep_idx, y, x, farm, args, bim, out, name)
        for mode in ((["lmm"] if args.lmm and ti not in lmm_done else []) + (["lmm2"] if args.lmm2 else []) +
                     (["fvlmm"] if args.fvlmm else [])):
            t1 = time.perf_counter()
            # rows are formatted and written block by block on a writer thread while the device scans the next block
            # (src/stats/lmm.rs:975-1477 with its AsyncTsvWriter, src/stats/common.rs:374)
            wr = {}

            def open_writer(keep_mask, af_k, miss_k, ncol, model_tag):
                kept_rows = np.nonzero(keep_mask)[0]
                wr["path"] = f"{out}.{name}.{model_tag}.tsv"
                wr["w"] = AsyncAssocTsvWriter(wr["path"], ncol, *bim.columns(kept_rows), af_k, miss_k,
                                              miss_count=(model_tag == "lm"))
                return wr["w"].put

            try:
                # `-lmm`: the reference's default scan -- warm-start chains over chunks of `-chunksize` rows of the file, seeded
                # with log10 lambda0 (workflow_model_stream.py:1436-1480; src/stats/lmm.rs:2627); JX_LMM_UNIFIED_NO_WARM_START=1
                # or `-warm-start none` give every SNP the same start (and the faster one-wave-per-SNP scan)
                chain = None
                if mode == "lmm" and _warm_start_mode(args) == "chain":
                    chain = (max(1, int(args.chunksize)), max(1, int(args.warm_chain_pieces)))
                res = pl.run_trait(packed_t, n_fam, k, keep_idx, y, x, mode, args.maf, args.geno, args.het,
                                   on_rows=open_writer, force_model=bool(args.force_model), warm_chain=chain)
            except BaseException:
                if "w" in wr:
                    wr["w"].abort()
                raise
            if "w" in wr:
                wr["w"].close()
            kept = np.nonzero(res.keep)[0]
            path = wr.get("path", f"{out}.{name}.{res.model_tag}.tsv")
            if res.model_tag == "lm":
                # LMM -> LM fallback (src/stats/gwas_unified.rs:121-175, workflow_model_stream.py:930-963)
                _sw, stat, pv = res.null_lrt
                print(f"[{name}] Warning: -{mode} switch to LM: null LRT stat={stat:.4g}, p={pv:.4g} (>=0.05); "
                      f"pve(null)={res.null.pve:.4f}")
                print(f"[{name}] -lm: n={n} snps={len(kept)} -> {path} ({time.perf_counter() - t1:.2f}s)")
            else:
                print(f"[{name}] -{mode}: n={n} snps={len(kept)} lambda0={res.null.lbd:.5g} pve={res.null.pve:.4f} "
                      f"-> {path} ({time.perf_counter() - t1:.2f}s)")
        if sparse_path is not None:
            from . import stats as st
            t1 = time.perf_counter()
            full = n == n_fam and np.array_equal(keep_idx, np.arange(n_fam))
            counts = jxrs.bed_row_counts(packed, n_fam, None if full else keep_idx)
            keep, af, miss = st.gwas_scan_row_stats(counts, n, args.maf, args.geno, args.het)
            kept = np.nonzero(keep)[0]
            maf_all = np.zeros(packed.shape[0], dtype=np.float32)
            maf_all[kept] = af[kept]
            grm_idx = None
            if sparse_pos is not None:
                missing_ids = [fam[j] for j in keep_idx if fam[j] not in sparse_pos]
                if missing_ids:
                    raise SystemExit(f"{sparse_path}.id lacks {len(missing_ids)} phenotyped sample(s), e.g. {missing_ids[0]}")
                grm_idx = np.array([sparse_pos[fam[j]] for j in keep_idx], dtype=np.int64)
            xc = x[:, 1:] if x.shape[1] > 1 else None
            sidx = keep_idx if (grm_idx is not None or not full) else None
            meta = bim.columns(kept)
            for stem in sp_stems:
                t2 = time.perf_counter()
                path = f"{out}.{name}.{stem}.tsv"
                approx = stem == "splmm" and len(kept) >= SPLMM_APPROX_RHAT_MARKERS
                if stem == "splmm" and not approx:
                    # python/janusx/assoc/workflow_model_packed.py:8087-8107
                    print(f"[{name}] Warning: SparseLMM approx scan has fewer filtered markers than the default gamma sample size "
                          f"({len(kept)} < {SPLMM_APPROX_RHAT_MARKERS}); falling back to splmm-exact for this trait.")
                if approx:
                    # null: fastGWA fixed-Vp objective on the OLS residual (workflow_model_packed.py:3134-3156, 3430-3451), then
                    # the residualised GRAMMAR-gamma scan (`splmm_assoc_pcg_bed_to_tsv`, scan_mode "approx", :8527-8563)
                    xd = np.ones((n, 1)) if xc is None else np.concatenate([np.ones((n, 1)), xc], axis=1)
                    yc = y - xd @ np.linalg.solve(xd.T @ xd, xd.T @ y)
                    yc = yc - float(np.mean(yc))
                    vp = float(yc @ yc) / float(n - 1)
                    null = jxrs.spreml_sparse_fastgwa_fixed_vp_brent_from_jxgrm(sparse_path, yc, vp, sample_indices=grm_idx if grm_idx is not None else sidx,
                                                                               low=-5.0, high=5.0, grid_size=17, tol=1e-3, max_iter=20)
                    res = jxrs.splmm_assoc_pcg_bed_to_tsv(args.bfile, y, float(null[0]), *meta, path, x_cov=xc, sample_indices=sidx,
                                                          packed=packed, packed_n_samples=n_fam, maf=af[kept], row_flip=np.zeros(len(kept), bool),
                                                          row_missing=miss[kept], row_indices=kept, sparse_sample_indices=grm_idx,
                                                          sparse_jxgrm_path=sparse_path, rhat_markers=SPLMM_APPROX_RHAT_MARKERS,
                                                          rhat_seed=20260527, scan_mode="approx")
                    print(f"[{name}] -splmm: n={n} snps={len(kept)} lambda0={null[0]:.5g} sigma_g2={null[1]:.4g} sigma_e2={null[2]:.4g} "
                          f"gamma={res[0]:.6g} (markers used {res[8]}) -> {path} ({time.perf_counter() - t2:.2f}s)")
                else:
                    stats, l10, null = jxrs.splmm_exact_scan_from_jxgrm(
                        sparse_path, y, packed, n_fam, maf_all, np.zeros(packed.shape[0], dtype=bool), xc, sidx, kept,
                        grid_size=17, tol=1e-3, max_iter=20, grm_sample_indices=grm_idx)
                    if rank == 0:
                        write_assoc_tsv(path, *meta, af[kept], miss[kept], stats)
                    print(f"[{name}] -{'splmm-exact' if stem == 'splmm2' else 'splmm (exact scan)'}: n={n} snps={len(kept)} "
                          f"lambda0={null[0]:.5g} sigma_g2={null[1]:.4g} sigma_e2={null[2]:.4g} -> {path} "
                          f"({time.perf_counter() - t2:.2f}s)")
    return 0


BLUP_SMALL_N = 15000      # python/janusx/gs/blup.py:8-9
BLUP_SMALL_M = 15000


def resolve_blup_dispatch(n_samples, n_markers, force=None):
    """`resolve_blup_dispatch` (python/janusx/gs/blup.py:73-163) -> (effective method, rrBLUP solver or None).  `force` = the
    value of GS_BLUP ("0" GBLUP, "1" exact rrBLUP, "2" PCG rrBLUP; None / "" = automatic)."""
    force = (force or "").strip()
    if force not in ("", "0", "1", "2"):
        raise ValueError(f"Invalid GS_BLUP={force!r}; expected 0 (GBLUP), 1 (rrBLUP exact), or 2 (rrBLUP PCG).")
    if force == "0":
        return "GBLUP", None
    if force == "1":
        return "rrBLUP", "exact"
    if force == "2":
        return "rrBLUP", "pcg"
    if max(0, int(n_samples)) <= BLUP_SMALL_N:
        return "GBLUP", None
    return "rrBLUP", ("exact" if max(0, int(n_markers)) <= BLUP_SMALL_M else "pcg")


def cmd_gs(args):
    """`jx gs -BLUP`: centred GRM of all genotyped samples (once), then per trait a GBLUP fit on the phenotyped
    samples (spectral REML, src/stats/gblup.rs:1105-1240) -- K-fold cross-validated with `-cv` (folds of
    `build_cv_splits`, seeded by `-seed` = 42, python/janusx/gs/workflow.py:3950-3980, 18753-18760) -- and predictions for every genotyped sample."""
    from . import janusx as jxrs
    from .bed import read_fam_ids
    if args.rrblup:
        return cmd_gs_rrblup(args)
    if not (args.blup or args.gblup):
        raise SystemExit("select a model: -BLUP (or -GBLUP, -rrBLUP)")
    fam = read_fam_ids(args.bfile)
    ids, names, ph = _read_table(args.pheno)
    pos = {s: i for i, s in enumerate(ids)}
    traits = _select_traits(names, args.ncol)
    if args.blup and not args.gblup:
        # -BLUP = automatic dispatch (`resolve_blup_dispatch`, python/janusx/gs/blup.py:8-163): n_train <= 15000 -> GBLUP;
        # beyond that rrBLUP, exact (marker space) up to 15000 kept markers and PCG above; GS_BLUP=0/1/2 forces a route
        force = os.environ.get("GS_BLUP", "").strip()
        n_train_max = 0
        for ti in traits:
            n_train_max = max(n_train_max, sum(1 for sid in fam if sid in pos and math.isfinite(ph[pos[sid], ti])))
        try:
            method, _solver = resolve_blup_dispatch(n_train_max, 0, force)
        except ValueError as e:
            raise SystemExit(str(e))
        if method == "rrBLUP":
            # the kept-marker count is known only behind the QC of the rrBLUP route: its "auto" solver applies the same
            # 15000-marker rule (exact up to it, PCG above)
            args.rr_solver = {"1": "exact", "2": "pcg"}.get(force, "auto")
            print(f"-BLUP dispatch: n_train={n_train_max} -> rrBLUP ({args.rr_solver})"
                  + (f" (forced by GS_BLUP={force})" if force else ""))
            return cmd_gs_rrblup(args)
        print(f"-BLUP dispatch: n_train={n_train_max} -> GBLUP" + (" (forced by GS_BLUP=0)" if force == "0" else ""))
    out = _resolve_out(args, args.bfile)
    t0 = time.perf_counter()
    if args.grm:
        k = _load_grm(args.grm, fam)
        print(f"GRM loaded from {args.grm}: n={k.shape[0]}")
    else:
        k, eff, _ = jxrs.grm_stream_bed_f32(args.bfile, method=1, maf_threshold=args.maf, max_missing_rate=args.geno,
                                            het_threshold=0.0)
        print(f"GRM method 1: n={k.shape[0]} eff_m={eff} ({time.perf_counter() - t0:.2f}s)")
    n_all = len(fam)
    for ti in traits:
        name = names[ti]
        yv = np.array([ph[pos[s], ti] if s in pos else np.nan for s in fam])
        train = np.nonzero(np.isfinite(yv))[0].astype(np.int64)
        test = np.nonzero(~np.isfinite(yv))[0].astype(np.int64)
        if len(train) < 10:
            print(f"[{name}] only {len(train)} phenotyped samples, skipped")
            continue
        t1 = time.perf_counter()
        fold = np.full(n_all, -1, dtype=np.int64)
        pred = np.full(n_all, np.nan)
        if args.cv and args.cv > 1:
            print("Fold Method     Pearsonr Spearmanr R2")
            for f, (te_loc, tr_loc) in enumerate(build_cv_splits(len(train), args.cv, args.seed)):
                r = jxrs.gblup_reml_grm(k, train[tr_loc], yv[train[tr_loc]], train[te_loc], estimate_only=False)
                pred[train[te_loc]] = r[1].ravel()
                fold[train[te_loc]] = f
                pe, sp, r2f = cv_fold_metrics(yv[train[te_loc]], r[1].ravel())
                print(f"{f + 1:<4d} BLUP       {pe:.3f}    {sp:.3f}     {r2f:.3f}")
            yo, po = yv[train], pred[train]
            rr = float(np.corrcoef(yo, po)[0, 1])
            r2 = 1.0 - float(np.sum((yo - po) ** 2) / np.sum((yo - yo.mean()) ** 2))
            print(f"[{name}] GBLUP {args.cv}-fold CV: pearson={rr:.4f} R2={r2:.4f}")
        full = jxrs.gblup_reml_grm(k, train, yv[train], test if len(test) else None, return_variance_components=True)
        if not (args.cv and args.cv > 1):
            pred[train] = full[0].ravel()
        if len(test):
            pred[test] = full[1].ravel()
        path = f"{out}.{name}.gs.GBLUP.tsv"
        tmp = f"{path}.tmp.{os.getpid()}"
        with open(tmp, "w") as fh:
            fh.write("sample\tobserved\tpredicted\tfold\n")
            for j, sid in enumerate(fam):
                obs = "NA" if not math.isfinite(yv[j]) else f"{yv[j]:.6g}"
                fh.write(f"{sid}\t{obs}\t{pred[j]:.6g}\t{'NA' if fold[j] < 0 else fold[j]}\n")
        os.replace(tmp, path)
        print(f"[{name}] GBLUP: n_train={len(train)} n_pred={len(test)} lambda={full[3]:.5g} pve={full[2]:.4f} "
              f"sigma_g2={full[9]:.5g} sigma_e2={full[10]:.5g} -> {path} ({time.perf_counter() - t1:.2f}s)")
    return 0


def cmd_gs_rrblup(args):
    """`jx gs -rrBLUP`: marker effects of the standardised genotypes, by the exact marker-space route
    (`rrblup_exact_snp_packed`, src/stats/rrblup.rs:3179-3490) or by PCG over the packed payload
    (`rrblup_pcg_bed`, src/stats/rrblup.rs:3494-4307; the route python/janusx/gs/blup.py:146-163 takes for large n
    and m).  lambda (equation scale, sigma_e^2 / sigma_beta^2) is `-lambda` when given; otherwise
    m_effective * sigma_e^2 / sigma_g^2 from the spectral GBLUP REML of a random subsample of at most 2000 training
    samples (seed `-seed`) on the standardised GRM -- the GRM-REML branch of the reference's
    `_estimate_rrblup_lambda_subsample_reml` (python/janusx/gs/workflow.py:5481) without its HE variants."""
    from . import janusx as jxrs
    from .bed import read_fam_ids
    fam = read_fam_ids(args.bfile)
    ids, names, ph = _read_table(args.pheno)
    pos = {s: i for i, s in enumerate(ids)}
    traits = _select_traits(names, args.ncol)
    out = _resolve_out(args, args.bfile)
    packed, miss, maf, _std, n_all = jxrs.load_bed_2bit_packed(args.bfile)
    flip = jxrs.bed_packed_row_flip_mask(packed, n_all)
    keep = (maf >= np.float32(args.maf)) & (miss <= np.float32(args.geno))
    # solver choice of the reference (`_resolve_rrblup_solver` + `_resolve_rrblup_exact_backend`, python/janusx/gs/workflow.py:
    # 5230-5276): up to 15 000 markers the exact marker-space route ("snp": REML lambda from the m x m spectrum); beyond that
    # the exact SAMPLE-space route ("fast": REML on the spectrum of the n x n kernel of the standardised markers) while the
    # phenotyped samples number at most 10 000, PCG above
    solver = args.rr_solver
    if solver in ("exact", "fast") and args.lam is not None:
        raise SystemExit("-lambda needs -rr-solver pcg: the exact routes estimate lambda by REML on the spectrum and would "
                         "ignore the given value")
    n_pheno_max = max((int(np.isfinite([ph[pos[s], ti] if s in pos else np.nan for s in fam]).sum()) for ti in traits), default=0)
    if solver == "auto":
        # a given -lambda only exists on the PCG route (the exact routes re-estimate it): honour it
        if args.lam is not None:
            solver = "pcg"
        elif int(keep.sum()) <= 15000:
            solver = "exact"
        else:
            solver = "fast" if n_pheno_max <= 10000 else "pcg"
    print(f"rrBLUP-{solver.upper()}: n={n_all} m={packed.shape[0]} kept={int(keep.sum())} (maf {args.maf}, geno {args.geno})")
    k_std = None
    if solver == "fast":
        # sample-space exact route (the reference's "fast" backend: pyBLUP.BLUP on the implicit kinship of the standardised
        # markers, python/janusx/pyBLUP/mlm.py): ridge regression on Z is GBLUP on K = Z'Z / m_eff with lambda_equation =
        # m_eff * sigma_e^2 / sigma_g^2.  K over ALL genotyped samples once (global allele frequencies, like the marker-space
        # routes), then per fit eigendecomposition of K[train, train] + Brent on its spectrum + K[test, train] alpha
        # (`gblup_reml_grm`: the kernels of the `-BLUP` branch)
        p_std = np.clip(maf[keep], 0.0, 0.5)
        m_eff_std = int(np.count_nonzero(2.0 * p_std * (1.0 - p_std) > 1e-12))
        t0k = time.perf_counter()
        k_std = jxrs.grm_packed_f32(np.ascontiguousarray(packed[keep]), n_all, flip[keep], maf[keep], None, method=2)
        print(f"standardised kernel of {n_all} samples over {m_eff_std} markers ({time.perf_counter() - t0k:.2f}s)")
    pcg_payload = packed
    if solver == "pcg":
        # the PCG route streams the payload from HBM for the whole solve: upload it ONCE and hand the device tensor to both
        # he_pcg_bed and rrblup_pcg_bed (their images of the training payload are shared inside `pcg_image_scope`)
        try:
            import warnings
            import torch
            if torch.cuda.is_available() and 3.2 * packed.nbytes < torch.cuda.mem_get_info()[0]:
                with warnings.catch_warnings():
                    # a read-only view of the mapped file: it is only read (copied to the device), never written through
                    warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
                    pcg_payload = torch.from_numpy(np.ascontiguousarray(packed)).cuda()
        except Exception:   # noqa: BLE001 - the host array works everywhere (uploaded per call)
            pcg_payload = packed
    for ti in traits:
        name = names[ti]
        yv = np.array([ph[pos[s], ti] if s in pos else np.nan for s in fam])
        train = np.nonzero(np.isfinite(yv))[0].astype(np.int64)
        test = np.nonzero(~np.isfinite(yv))[0].astype(np.int64)
        if len(train) < 10:
            print(f"[{name}] only {len(train)} phenotyped samples, skipped")
            continue
        t1 = time.perf_counter()
        scope = jxrs.pcg_image_scope() if solver == "pcg" else contextlib.nullcontext()
        with scope:   # the images are released when the block is left, also by an exception
            if solver in ("exact", "fast"):
                lam, src = None, "REML on the spectrum"
            elif args.lam is not None:
                lam, src = float(args.lam), "manual"
            elif not args.lambda_reml:
                # Haseman-Elston first (python/janusx/gs/workflow.py:5564 `he_first`): lambda_equation = lambda_k * m_effective
                try:
                    he = jxrs.he_pcg_bed("", train, yv[train], site_keep=keep, seed=args.seed if args.seed != 42 else 20260512,
                                         packed=pcg_payload, packed_n_samples=n_all, maf=maf, row_flip=flip)
                except RuntimeError as e:   # e.g. the stochastic traces violate the PSD bound on a small panel
                    he = None
                    lam, src = None, f"HE failed ({e})"
                if he is not None:
                    if np.isfinite(he[10]) and he[10] >= 0.0:
                        lam, src = max(1e-8, float(he[10]) * float(max(1, he[6]))), f"HE (h2={he[2]:.4f}, lambda_k={he[10]:.5g})"
                    else:
                        lam, src = None, "HE on the boundary"
            else:
                lam, src = None, ""
            if lam is None and solver == "pcg":
                rng = np.random.default_rng(args.seed)
                sub = np.sort(rng.permutation(len(train))[:min(len(train), 2000)])
                ks = jxrs.grm_packed_f32(np.ascontiguousarray(packed[keep]), n_all, flip[keep], maf[keep], train[sub], method=2)
                fit = jxrs.gblup_reml_grm(ks, np.arange(len(sub), dtype=np.int64), yv[train[sub]], None,
                                          return_variance_components=True)
                lam_k = float(fit[3])
                p = np.clip(maf[keep], 0.0, 0.5)
                m_eff = int(np.count_nonzero(2.0 * p * (1.0 - p) > 1e-12))
                lam, src = lam_k * m_eff, (src + " -> " if src else "") + f"subsample REML (n_sub={len(sub)}, lambda_k={lam_k:.5g})"
            fold = np.full(n_all, -1, dtype=np.int64)
            pred = np.full(n_all, np.nan)

            def fit_predict(tr, te):
                if solver == "fast":
                    r = jxrs.gblup_reml_grm(k_std, tr, yv[tr], te if len(te) else None, return_variance_components=True)
                    # (pred_train, pred_test, pve, lambda_k, ml, reml, ..., sigma_g2, sigma_e2): same slots as the marker-space fit
                    return (r[0], r[1], r[2], float(r[3]) * float(m_eff_std), r[5], (r[9], r[10]), m_eff_std)
                if solver == "exact":
                    return jxrs.rrblup_exact_snp_packed(packed, n_all, tr, yv[tr], te if len(te) else None, site_keep=keep,
                                                        maf=maf, row_flip=flip)
                return jxrs.rrblup_pcg_bed("", tr, yv[tr], te if len(te) else None, site_keep=keep, lambda_value=lam,
                                           tol=args.tol, max_iter=args.max_iter, packed=pcg_payload, packed_n_samples=n_all,
                                           maf=maf, row_flip=flip)

            if args.cv and args.cv > 1:
                print("Fold Method     Pearsonr Spearmanr R2")
                for f, (te_loc, tr_loc) in enumerate(build_cv_splits(len(train), args.cv, args.seed)):
                    r = fit_predict(train[tr_loc], train[te_loc])
                    pred[train[te_loc]] = r[1].ravel()
                    fold[train[te_loc]] = f
                    pe, sp, r2f = cv_fold_metrics(yv[train[te_loc]], r[1].ravel())
                    print(f"{f + 1:<4d} rrBLUP     {pe:.3f}    {sp:.3f}     {r2f:.3f}")
                yo, po = yv[train], pred[train]
                rr = float(np.corrcoef(yo, po)[0, 1])
                r2 = 1.0 - float(np.sum((yo - po) ** 2) / np.sum((yo - yo.mean()) ** 2))
                print(f"[{name}] rrBLUP {args.cv}-fold CV: pearson={rr:.4f} R2={r2:.4f}")
            full = fit_predict(train, test)
        if not (args.cv and args.cv > 1):
            pred[train] = full[0].ravel()
        if len(test):
            pred[test] = full[1].ravel()
        path = f"{out}.{name}.gs.rrBLUP.tsv"
        tmp = f"{path}.tmp.{os.getpid()}"
        with open(tmp, "w") as fh:
            fh.write("sample\tobserved\tpredicted\tfold\n")
            for j, sid in enumerate(fam):
                obs = "NA" if not math.isfinite(yv[j]) else f"{yv[j]:.6g}"
                fh.write(f"{sid}\t{obs}\t{pred[j]:.6g}\t{'NA' if fold[j] < 0 else fold[j]}\n")
        os.replace(tmp, path)
        if solver in ("exact", "fast"):
            print(f"[{name}] rrBLUP-{'EXACT' if solver == 'exact' else 'FAST (sample space)'}: n_train={len(train)} n_pred={len(test)} lambda={full[3]:.5g} [{src}] "
                  f"reml={full[4]:.6g} var_g={full[5][0]:.5g} sigma_e2={full[5][1]:.5g} m_effective={full[6]} "
                  f"pve={full[2]:.4f} -> {path} ({time.perf_counter() - t1:.2f}s)")
        else:
            print(f"[{name}] rrBLUP-PCG: n_train={len(train)} n_pred={len(test)} lambda={lam:.5g} [{src}] "
                  f"converged={full[3]} iters={full[4]} rel_res={full[5]:.3g} m_effective={full[6]} "
                  f"pve={full[7]:.4f} -> {path} ({time.perf_counter() - t1:.2f}s)")
    return 0


def _resolve_pca_grm(spec):
    """-k PATH or PREFIX (python/janusx/script/pca.py:1720-1760): PREFIX.cGRM.npy / .sGRM.npy / .grm.npy (then .txt); sample ids
    from {file}.id -> (path, ids)."""
    cands = [spec] + [f"{spec}.{t}.{e}" for e in ("npy", "txt") for t in ("cGRM", "sGRM", "grm")]
    path = next((c for c in cands if os.path.isfile(c)), None)
    if path is None:
        raise SystemExit(f"GRM not found: {spec} (tried {', '.join(cands)})")
    if not os.path.exists(path + ".id"):
        raise SystemExit(f"{path}.id not found (sample ids of the GRM)")
    ids = [ln.split()[0] for ln in open(path + ".id") if ln.strip()]
    return path, ids


def _write_pca(out, ids, eigvec, eigval, dim, total_variance=None):
    """{out}.eigenvec (id + the first `dim` columns, %.6f, tab, no header; pca.py:1700-1716) and {out}.eigenval (eigenvalue,
    explained ratio, %.8f, tab; `_write_eigenval_table`, pca.py:795-820)."""
    ev = np.asarray(eigval, dtype=np.float64).reshape(-1)
    total = float(np.sum(ev)) if total_variance is None else float(total_variance)
    ratio = ev / total if (np.isfinite(total) and total > 0.0) else np.zeros_like(ev)
    vec = np.asarray(eigvec, dtype=np.float64)[:, :dim]
    with open(f"{out}.eigenvec", "w") as fh:
        for sid, row in zip(ids, vec):
            fh.write("\t".join([str(sid)] + ["%.6f" % v for v in row]) + "\n")
    np.savetxt(f"{out}.eigenval", np.column_stack([ev, ratio]), fmt=["%.8f", "%.8f"], delimiter="\t")


_PRUNE_UNITS = (("kb", 1000.0, " (kb)"), ("bp", 1.0, " (bp)"))   # suffix of a physical window, base pairs per unit, error tag


def _parse_prune_window(token):
    """WINDOW of `-prune` -> (window_variants, window_bp), one of them None.  Behaviour and messages of the reference's parser
    (python/janusx/script/gformat.py:617-641): case and blanks are ignored; `kb` / `bp` suffixes give a physical window in base
    pairs, rounded and at least 1; a bare number is a variant count and must be a whole number."""
    text = str(token).strip().lower()
    if not text:
        raise ValueError("Empty prune window token.")
    for suffix, scale, tag in _PRUNE_UNITS:
        if text.endswith(suffix):
            size = float(text[:-len(suffix)].strip())
            if not (np.isfinite(size) and size > 0):
                raise ValueError(f"Invalid prune window{tag}: {token}")
            return None, max(1, int(round(size * scale)))
    count = float(text)
    if not (np.isfinite(count) and count > 0):
        raise ValueError(f"Invalid prune window: {token}")
    whole = int(round(count))
    if abs(count - whole) > 1e-9:
        raise ValueError(f"Invalid prune window: {token}. Use an integer variant count, "
                         "or add kb/bp suffix for a physical window.")
    return max(1, whole), None


def _parse_prune_args(values):
    """`-prune WINDOW STEP R2` -> (window_variants, window_bp, step_variants, r2_threshold); None when the flag is absent.
    Behaviour and messages of python/janusx/script/gformat.py:644-664: STEP is a number truncated to an integer > 0, R2 a finite
    number in (0, 1]."""
    if values is None:
        return None
    if len(values) != 3:
        raise ValueError("Invalid --prune usage. Expected 3 values: "
                         "--prune <window size['kb']> <step size (variant ct)> <r^2 threshold>")
    window, step_text, r2_text = values
    variants, bp = _parse_prune_window(window)
    step = int(float(str(step_text).strip()))
    if step < 1:
        raise ValueError(f"--prune step must be > 0, got {step_text!r}")
    r2 = float(str(r2_text).strip())
    if not (np.isfinite(r2) and 0.0 < r2 <= 1.0):
        raise ValueError(f"--prune r^2 threshold must be in (0, 1], got {r2_text!r}")
    return variants, bp, step, r2


def _prune_chrom_codes(chroms):
    """Consecutive integers by first appearance of the `.bim` chromosome string (python/janusx/script/gformat.py:1509-1519)."""
    codes, out = {}, np.zeros(len(chroms), dtype=np.int32)
    for i, c in enumerate(chroms):
        out[i] = codes.setdefault(str(c), len(codes))
    return out


def cmd_gformat(args):
    """`jx gformat -bfile PREFIX -prune WINDOW STEP R2` (python/janusx/script/gformat.py:1456-1546, 2563-2575): LD pruning with MAF
    priority (`bed_packed_ld_prune_maf_priority`) and the pruned PLINK set written beside the project's other outputs.  The other
    conversions and filters of the reference's gformat, and its external-PLINK backend, are not built."""
    for flag, what in (("vcf", "-vcf"), ("hmp", "-hmp"), ("file", "-file")):
        if getattr(args, flag, None):
            raise SystemExit(f"gformat: {what} input is not supported on this build; give a PLINK prefix with -bfile")
    for flag, what in (("format", "-fmt"), ("maf", "-maf"), ("geno", "-geno"), ("het", "-het"), ("keep", "-keep"),
                       ("extract", "-extract"), ("snps_only", "-snps-only"), ("biallelic_only", "-biallelic-only"),
                       ("snp_name", "-snp-name"), ("chr", "-chr"), ("from_bp", "-from-bp"), ("to_bp", "-to-bp")):
        if getattr(args, flag, None) not in (None, False):
            raise SystemExit(f"gformat: {what} (format conversion and site / sample filters) is out of scope on this build; "
                             "only -bfile PREFIX -prune WINDOW STEP R2 is built")
    if os.environ.get("JX_LD_PRUNE_BACKEND", "").strip().lower() in ("plink", "plink-external", "external-plink"):
        raise SystemExit("gformat: the external PLINK prune backend (JX_LD_PRUNE_BACKEND) is out of scope on this build")
    if not args.bfile:
        raise SystemExit("gformat needs -bfile PREFIX")
    try:
        spec = _parse_prune_args(args.prune)
    except ValueError as e:
        raise SystemExit(f"gformat: {e}") from None
    if spec is None:
        raise SystemExit("gformat: only LD pruning is built; give -prune WINDOW STEP R2")
    w_var, w_bp, step, r2 = spec
    rank, _world = _dist_setup()
    if rank != 0:                                             # one GPU does the work
        return 0
    from . import janusx as jxrs
    from .bed import read_bed_payload, read_fam_ids, write_bed
    src = jxrs._bed_prefix(args.bfile)
    out = _resolve_out(args, src)
    if os.path.abspath(out) == os.path.abspath(src):
        raise SystemExit(f"gformat: the output prefix {out} is the input; give another with -o / -prefix")
    t0 = time.perf_counter()
    packed, n, bim = read_bed_payload(src)
    packed = np.ascontiguousarray(packed)
    keep = jxrs.bed_packed_ld_prune_maf_priority(packed, n, _prune_chrom_codes(bim.chrom), np.asarray(bim.pos, dtype=np.int64),
                                                 window_bp=w_bp, window_variants=w_var, step_variants=step, r2_threshold=r2)
    rows = np.nonzero(keep)[0]
    with open(f"{src}.bim") as fh:
        bim_lines = [ln for ln in fh if len(ln.split()) >= 6]    # the rows `read_bim` keeps
    if len(bim_lines) != len(keep):
        raise SystemExit(f"gformat: {src}.bim has {len(bim_lines)} variant lines, the keep mask {len(keep)} rows")
    write_bed(out, packed[rows], read_fam_ids(src), bim.take(rows))
    # `write_bed` makes the .fam from ids alone and the .bim with a zero map distance: put the input's own lines back
    with open(f"{out}.bim", "w") as fh:
        fh.writelines(bim_lines[i] for i in rows)
    with open(f"{src}.fam") as fi, open(f"{out}.fam", "w") as fo:
        fo.write(fi.read())
    window = f"{w_bp}bp" if w_bp is not None else f"{w_var} variants"
    print(f"gformat: LD prune window={window}, step={step}, r2={r2:.4f}: kept {len(rows)} / {len(keep)} variants "
          f"({time.perf_counter() - t0:.2f} s) -> {out}.bed/.bim/.fam")
    return 0


def _parse_ldsc_window(text):
    """WINDOW of `jx gstats -ldsc` -> (kind, value, label): `_parse_ldsc_window` of python/janusx/script/gstats.py:100-138 with its
    grammar, labels and messages.  A bare number (or `snp` / `snps`) counts variants, `b` / `bp` / `kb` / `mb` are base pairs, `cm`
    genetic distance; nothing given means 100kb."""
    import re
    raw = "100kb" if text is None or str(text).strip() == "" else str(text).strip().lower()
    compact = raw.replace(" ", "")
    mt = re.fullmatch(r"([0-9]*\.?[0-9]+)([a-z]*)", compact)
    if mt is None:
        raise ValueError(f"Invalid -ldsc window: {text!r}. Use forms like 100, 100kb, 0.1mb, 100000b, or 10cm.")
    value, unit = float(mt.group(1)), str(mt.group(2) or "")
    if not math.isfinite(value) or value <= 0.0:
        raise ValueError(f"-ldsc window must be > 0, got {text!r}.")
    if unit in ("", "snp", "snps"):
        if not value.is_integer():
            raise ValueError(f"SNP-count LD-score window must be an integer, got {text!r}.")
        v = int(round(value))
        return "variants", float(v), f"{v}snp"
    if unit in ("b", "bp"):
        bp = int(round(value))
        return "bp", float(bp), f"{bp}b"
    if unit == "kb":
        return "bp", float(int(round(value * 1000.0))), compact
    if unit == "mb":
        return "bp", float(int(round(value * 1_000_000.0))), compact
    if unit == "cm":
        return "cm", float(value), compact
    raise ValueError(f"Unsupported -ldsc unit in {text!r}. Use forms like 100, 100kb, 0.1mb, 100000b, or 10cm.")


def _gstats_write_tables(src_path, min_cols, cols, out, tables, header):
    """One text table per (suffix, name, values) of `tables`: `header` and the name, then per non-blank line of `src_path` its
    columns `cols` copied as text and the value as `%.6f` (python/janusx/script/gstats.py:183-304)."""
    kind = "BIM" if src_path.endswith(".bim") else "FAM"
    expected = len(tables[0][2])
    with contextlib.ExitStack() as stack:
        outs = []
        for suffix, name, values in tables:
            fh = stack.enter_context(open(f"{out}.{suffix}", "w", encoding="utf-8"))
            fh.write(f"{header}\t{name}\n")
            outs.append((fh, values))
        row = 0
        with open(src_path, encoding="utf-8") as src:
            for line_no, line in enumerate(src, 1):
                if not line.strip():
                    continue
                toks = line.split()
                if len(toks) < min_cols:
                    raise SystemExit(f"gstats: Malformed {kind} file: {src_path}:{line_no}")
                if row >= expected:
                    raise SystemExit(f"gstats: {src_path} has more rows than the statistics ({row + 1} > {expected})")
                lead = "\t".join(toks[c].strip() for c in cols)
                for fh, values in outs:
                    fh.write(f"{lead}\t{float(values[row]):.6f}\n")
                row += 1
        if row != expected:
            raise SystemExit(f"gstats: {src_path} has {row} rows, the statistics {expected}")
    return [f"{out}.{suffix}" for suffix, _n, _v in tables]


def cmd_gstats(args):
    """`jx gstats -bfile PREFIX [-freq] [-miss] [-het] [-ldsc [WINDOW]]` (python/janusx/script/gstats.py:545-793): site MAF /
    missing / het tables, sample missing / het tables and windowed LD scores, with the reference's file names and text.  Its PDFs
    and its `.gstats.log` are not written (plots are out of scope on this build); non-BED input is refused."""
    for flag, what in (("vcf", "-vcf"), ("hmp", "-hmp"), ("file", "-file")):
        if getattr(args, flag, None):
            raise SystemExit(f"gstats: {what} input is not supported on this build; give a PLINK prefix with -bfile")
    if not args.bfile:
        raise SystemExit("gstats needs -bfile PREFIX")
    if not (args.freq or args.miss or args.het or args.ldsc is not None):
        raise SystemExit("gstats: select at least one statistic: -freq / -miss / -het / -ldsc")
    try:
        spec = _parse_ldsc_window(args.ldsc) if args.ldsc is not None else None
    except ValueError as e:
        raise SystemExit(f"gstats: {e}") from None
    rank, _world = _dist_setup()
    if rank != 0:                                             # one GPU does the work
        return 0
    from . import janusx as jxrs
    src = jxrs._bed_prefix(args.bfile)
    out = _resolve_out(args, src)
    t0 = time.perf_counter()
    outputs = []
    try:
        if args.freq or args.miss or args.het:
            if args.freq and not args.miss and not args.het:
                maf, lmiss, lhet, _n = jxrs.gstats_bed_site_stats(src)
                imiss = ihet = None
            else:
                maf, lmiss, lhet, imiss, ihet, _n, _m = jxrs.gstats_bed_joint_stats(
                    src, site_maf=bool(args.freq), site_miss=bool(args.miss), site_het=bool(args.het),
                    individual_miss=bool(args.miss), individual_het=bool(args.het))
            site = [t for t, on in ((("freq", "freq", maf), args.freq), (("lmiss", "miss", lmiss), args.miss),
                                    (("lhet", "het", lhet), args.het)) if on]
            outputs += _gstats_write_tables(f"{src}.bim", 4, (0, 3), out, site, "chr\tpos")
            sample = [t for t, on in ((("imiss", "miss", imiss), args.miss), (("ihet", "het", ihet), args.het)) if on]
            if sample:
                outputs += _gstats_write_tables(f"{src}.fam", 2, (0, 1), out, sample, "fid\tiid")
        if spec is not None:
            kind, value, label = spec
            m_counts, ldsc, n = jxrs.gstats_bed_ldscore(src, kind, value)
            path = f"{out}.{int(n)}.{label}.ldsc"
            with open(f"{src}.bim", encoding="utf-8") as fh:
                sites = [(t[0].strip(), int(t[3])) for t in (ln.split() for ln in fh) if t]
            with open(path, "w", encoding="utf-8") as fh:
                fh.write("chr\tpos\tM\tldsc\n")
                fh.writelines(f"{c}\t{p}\t{int(k)}\t{float(v):.6f}\n" for (c, p), k, v in zip(sites, m_counts, ldsc))
            outputs.append(path)
    except RuntimeError as e:
        raise SystemExit(f"gstats: {e}") from None
    print(f"gstats: finished in {time.perf_counter() - t0:.2f} s (the reference's PDF plots and .gstats.log are not written on this "
          "build)")
    for path in outputs:
        print(f"  {path}")
    return 0


def cmd_pca(args):
    """`jx pca` (python/janusx/script/pca.py:1134-1265): -bfile -> method-1 GRM with QC and its eigendecomposition, or with -rsvd
    the randomized SVD of the genotypes (`admx_rsvd_stream_sample`); -k -> eigendecomposition of a GRM file."""
    for flag, what in (("vcf", "-vcf"), ("hmp", "-hmp"), ("file", "-file")):
        if getattr(args, flag, None):
            raise SystemExit(f"pca: {what} input is not supported on this build; give a PLINK prefix with -bfile")
    for flag, what in (("qcov", "-c/--qcov"), ("plot", "-plot"), ("plot3d", "-plot3D"), ("group", "-group"),
                       ("palette", "-palette")):
        if getattr(args, flag, None):
            raise SystemExit(f"pca: {what} (plots and the view-only mode) is out of scope on this build")
    if bool(args.bfile) == bool(args.grm):
        raise SystemExit("pca needs exactly one of -bfile PREFIX or -k GRM")
    rsvd = args.rsvd is not None
    power, tol = 3, 0.1
    if rsvd:
        if args.grm:
            raise SystemExit("pca: -rsvd works on genotype input (-bfile), not on a GRM (-k)")
        if len(args.rsvd) > 2:
            raise SystemExit("-rsvd accepts at most two optional values: [power] [tol].")
        try:
            if len(args.rsvd) >= 1:
                power = int(args.rsvd[0])
            if len(args.rsvd) >= 2:
                tol = float(args.rsvd[1])
        except ValueError:
            raise SystemExit("Invalid -rsvd values: use '-rsvd 3' or '-rsvd 3 0.1' (power integer >= 0, tol > 0)") from None
        if power < 0:
            raise SystemExit("RSVD power must be >= 0.")
        if not tol > 0:
            raise SystemExit("RSVD tol must be > 0.")
    if args.dim < 1:
        raise SystemExit(f"pca: -dim must be >= 1 (got {args.dim})")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("PCA runs on one GPU: start it without the launcher")
    import torch
    from . import janusx as jxrs
    from . import pipeline as pl
    from .bed import read_fam_ids, snps_only_mask, stage_bed_payload
    out = _resolve_out(args, args.bfile or args.grm)
    t0 = time.perf_counter()
    total_variance = None
    if args.grm:
        path, ids = _resolve_pca_grm(args.grm)
        k = np.loadtxt(path, dtype=np.float64) if path.lower().endswith(".txt") else np.load(path)
        if k.ndim != 2 or k.shape != (len(ids), len(ids)):
            raise SystemExit(f"GRM shape {k.shape} does not match the {len(ids)} ids of {path}.id")
        s, ut = pl.eigh_from_grm(torch.from_numpy(np.ascontiguousarray(k)).to(torch.device("cuda", torch.cuda.current_device())),
                                 ridge=0.0)
        eigval, eigvec = s.cpu().numpy()[::-1], ut.cpu().numpy()[::-1].T
        what = f"GRM {path}"
    else:
        ids = read_fam_ids(args.bfile)
        packed_t, n, bim = stage_bed_payload(args.bfile, None)
        if rsvd:
            ev, vec, total_variance, rounds = jxrs._admx_rsvd(args.bfile, args.dim, 42, power, tol, bool(args.snps_only),
                                                              args.maf, args.geno, payload=(packed_t, n, bim))
            eigval, eigvec = ev.astype(np.float64), vec
            what = f"randomized SVD ({rounds} power rounds)"
        else:
            if args.snps_only:
                packed_t = packed_t[torch.from_numpy(np.nonzero(snps_only_mask(bim))[0]).to(packed_t.device)]
            k_t, eff, _ = pl.build_grm(packed_t, n, 1, args.maf, args.geno)
            s, ut = pl.eigh_from_grm(k_t, ridge=0.0)
            eigval, eigvec = s.cpu().numpy()[::-1], ut.cpu().numpy()[::-1].T
            what = f"GRM method 1 (eff_m={eff})"
    dim = min(int(args.dim), eigvec.shape[1])
    _write_pca(out, ids, eigvec, eigval, dim, total_variance)
    print(f"PCA: {what}, n={len(ids)} dim={dim} -> {out}.eigenvec, {out}.eigenval ({time.perf_counter() - t0:.2f}s)")
    return 0


ADMX_DEFAULTS = dict(power=5, max_als=1000, reg_als=1e-5, lr=0.005, beta1=0.80, beta2=0.88, epsilon=1e-8, lr_decay=0.5,
                     min_lr=1e-6)     # python/janusx/script/adamixture.py (the CLI's fixed optimiser settings)


ADMX_CV_MAX_FOLDS = 256    # janusx.ADMX_CV_MAX_FOLDS (the argument checks run before that module and torch are imported)
CVERROR_COLUMNS = ("K", "CVerror", "CVerror_SE", "CV_folds", "WallTime_sec", "Q_output", "P_npy_output", "P_site_output",
                   "Structure_plot", "Log_file")


def write_cverror_summary_tsv(path, rows):
    """`_write_cverror_summary_tsv` (python/janusx/script/adamixture.py:1096-1135): one line per K of dicts with k, cverror,
    cverror_se, cv_folds, wall, q_out, p_npy_out, p_site_out, log_path; the Structure_plot column stays empty (no plots)."""
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\t".join(CVERROR_COLUMNS) + "\n")
        for r in rows:
            fh.write("\t".join([str(int(r["k"])), f"{float(r['cverror']):.6f}", f"{float(r['cverror_se']):.6f}",
                                str(int(r["cv_folds"])), f"{float(r['wall']):.3f}", str(r["q_out"]), str(r["p_npy_out"]),
                                str(r["p_site_out"]), "", str(r["log_path"])]) + "\n")


def _k_range(tok, lo_s, hi_s, step_s):
    lo, hi = int(lo_s), int(hi_s)
    step = abs(int(step_s)) if step_s is not None else 1
    if step == 0:
        raise ValueError(f"K range step must be non-zero: {tok!r}")
    if hi < lo:
        step = -step
    return list(range(lo, hi + (1 if step > 0 else -1), step))


def parse_k_spec(spec):
    """The -k grammar of `jx adamixture` (`_parse_k_spec`, python/janusx/script/adamixture.py:1027-1093): a value (8), an
    inclusive range (1..10 or 1:10), a stepped range (1..10..3, 1:10:3, 1..10:3), a comma list, or a mix of these; duplicates
    dropped in first-seen order, every K >= 1.  Raises ValueError."""
    text = str(spec if spec is not None else "").strip()
    if not text:
        raise ValueError("Empty -k/--k specification.")
    if ";" in text:
        raise ValueError("Semicolon-separated K list is not supported for shell compatibility. Use comma-separated form, "
                         "e.g. -k 1,5,8.")
    toks = [t.strip() for t in text.split(",") if t.strip()]
    if not toks:
        raise ValueError(f"Invalid -k/--k specification: {spec!r}")
    vals = []
    for tok in toks:
        if ".." in tok or ":" in tok:
            if ".." in tok:
                parts = [x.strip() for x in tok.replace("..", ":").split(":") if x.strip()]
            else:
                parts = tok.split(":")
            if len(parts) not in (2, 3):
                raise ValueError(f"Invalid K range token: {tok!r}")
            vals += _k_range(tok, parts[0], parts[1], parts[2] if len(parts) == 3 else None)
        else:
            vals.append(int(tok))
    if not vals:
        raise ValueError(f"Invalid -k/--k specification: {spec!r}")
    out = []
    for v in vals:
        if v < 1:
            raise ValueError(f"K must be >= 1, got {v}.")
        if v not in out:
            out.append(v)
    return out


def _admx_check_args(args):
    """Input and range checks of `jx adamixture` / `jx fastpop` -> the K list (SystemExit with a message on a refusal)."""
    cmd = args.cmd
    for flag, what in (("vcf", "-vcf"), ("hmp", "-hmp"), ("file", "-file")):
        if getattr(args, flag, None):
            raise SystemExit(f"{cmd}: {what} input is not supported on this build; give a PLINK prefix with -bfile")
    if not args.bfile:
        raise SystemExit(f"{cmd} needs -bfile PREFIX")
    if args.cv is not None and int(args.cv) >= 2:
        raise SystemExit(f"{cmd}: -cv {args.cv} is not accepted; the cross-validation error is spelled -cverror {args.cv} on this "
                         "build (use -cv 0 or leave it out)")
    if args.cv is not None and int(args.cv) < 0:
        raise SystemExit("-cv must be >= 0.")
    cve = getattr(args, "cverror", None)
    if cve is not None and int(cve) != 0 and not 2 <= int(cve) <= ADMX_CV_MAX_FOLDS:
        raise SystemExit(f"{cmd}: -cverror {cve} is out of range: 0 (off) or 2 <= folds <= {ADMX_CV_MAX_FOLDS} (the limit of this "
                         "build)")
    if not (0.0 <= float(args.maf) <= 0.5):
        raise SystemExit("-maf must be within [0, 0.5].")
    if not (0.0 <= float(args.geno) <= 1.0):
        raise SystemExit("-geno must be within [0, 1.0].")
    if not float(args.tol) > 0:
        raise SystemExit("-tol/--tol must be > 0.")
    if int(args.max_iter) <= 0:
        raise SystemExit("-max-iter/--max-iter must be a positive integer.")
    if int(args.check) <= 0:
        raise SystemExit("-check/--check must be a positive integer.")
    if args.thread is not None and int(args.thread) <= 0:
        raise SystemExit("-t/--thread must be a positive integer.")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{cmd} runs on one GPU: start it without the launcher")
    try:
        ks = parse_k_spec(args.k)
    except ValueError as e:
        raise SystemExit(f"{cmd}: {e}") from None
    bad = [k for k in ks if k > 64]
    if bad:
        raise SystemExit(f"{cmd}: K={bad[0]} is out of range: this build supports 1 <= K <= 64")
    return ks


def cmd_adamixture(args):
    """`jx adamixture` / `jx fastpop` (python/janusx/script/adamixture.py; fastpop.py is the same command): ancestry estimation
    by ALS + Adam-EM on the kept rows of a PLINK prefix (`AdmxBedTrainingSession.fit_k`), every K of the -k spec on one staged
    session.  Per K: {prefix}.{K}.Q.txt, .P.npy, .P.site, .fastpop.log; then {prefix}.fastpop.summary.log.  With -cverror N every K
    is followed by its N-fold cross-validation error (`admx_evaluate_cverror`), and {prefix}.fastpop.cverror.summary.tsv and the
    K of the smallest error close the scan."""
    ks = _admx_check_args(args)
    from . import janusx as jxrs
    from .bed import read_fam_ids, stage_bed_payload
    prefix_in = args.bfile[:-4] if args.bfile.lower().endswith((".bed", ".bim", ".fam")) else args.bfile
    outdir = args.out or "."
    os.makedirs(outdir, exist_ok=True)
    prefix = args.prefix or os.path.basename(prefix_in)
    ids = read_fam_ids(prefix_in)
    t0 = time.perf_counter()
    payload = stage_bed_payload(prefix_in, None)
    sess = jxrs.AdmxBedTrainingSession(prefix_in, bool(args.snps_only), float(args.maf), float(args.geno), 0, payload=payload)
    del payload
    t_stage = time.perf_counter() - t0
    summary = []
    cv_folds = int(args.cverror or 0)
    cv_rows = []
    fit_settings = (args.solver, ADMX_DEFAULTS["power"], float(args.tol), ADMX_DEFAULTS["max_als"], ADMX_DEFAULTS["reg_als"],
                    ADMX_DEFAULTS["lr"], ADMX_DEFAULTS["beta1"], ADMX_DEFAULTS["beta2"], ADMX_DEFAULTS["epsilon"],
                    int(args.max_iter), int(args.check), ADMX_DEFAULTS["lr_decay"], ADMX_DEFAULTS["min_lr"])
    for idx, k in enumerate(ks, 1):
        t1 = time.perf_counter()
        p, q, ll, it, init_ll, als_it = sess.fit_k(k, int(args.seed), *fit_settings)
        dt = time.perf_counter() - t1
        cv = None
        if cv_folds:
            t2 = time.perf_counter()
            try:
                cv = jxrs.admx_evaluate_cverror(sess, k, cv_folds, int(args.seed), *fit_settings)
            except ValueError as e:
                raise SystemExit(f"{args.cmd}: {e}") from None
            dt_cv = time.perf_counter() - t2
        base = os.path.join(outdir, f"{prefix}.{k}")
        with open(f"{base}.Q.txt", "w") as fh:
            for sid, row in zip(ids, q.astype(np.float64)):
                fh.write(sid + "\t" + "\t".join(f"{float(v):.8f}" for v in row) + "\n")
        np.save(f"{base}.P.npy", np.ascontiguousarray(p, dtype=np.float32))
        sess.write_site_file(f"{base}.P.site")
        with open(f"{base}.fastpop.log", "w") as fh:
            fh.write(f"command: {args.cmd}\n")
            fh.write(f"genotype: {prefix_in}\n")
            fh.write(f"K scan progress: {idx}/{len(ks)} (K={k}, spec={args.k})\n")
            fh.write(f"samples: {sess.n_samples}\nkept SNPs: {sess.n_snps} (maf >= {args.maf}, missing rate <= {args.geno}, "
                     f"snps-only {'on' if args.snps_only else 'off'})\n")
            fh.write(f"solver: {args.solver}  seed: {args.seed}  tol: {args.tol}  max-iter: {args.max_iter}  check: {args.check}\n")
            fh.write(f"ALS rounds: {als_it}  init log-likelihood: {init_ll:.6f}\n")
            fh.write(f"Adam-EM iterations: {it}  final log-likelihood: {ll:.6f}\n")
            fh.write(f"time: {dt:.3f} s (staging {t_stage:.3f} s, shared by the K scan)\n")
            if cv is not None:
                fh.write(f"CVerror: estimating from {cv_folds} folds (observed={cv['cv_observed']}, SNPs={sess.n_snps}, "
                         f"samples={sess.n_samples})\n")
                fh.write("CV fold sizes: " + ", ".join(f"F{i + 1}={int(c)}" for i, c in enumerate(cv["fold_counts"])) + "\n")
                fh.write(f"CVerror: {cv['cverror']:.6f} (SE={cv['cverror_se']:.6f}, folds={cv_folds})\n")
                fh.write("CV eval counts: " + ", ".join(f"F{i + 1}={int(c)}" for i, c in enumerate(cv["fold_eval_counts"])) + "\n")
                fh.write(f"CV time: {dt_cv:.3f} s\n")
            fh.write("structure plot: not drawn (plots are not built)\n")
            fh.write(f"outputs: {base}.Q.txt {base}.P.npy {base}.P.site\n")
        summary.append((k, ll, init_ll, it, als_it, dt))
        print(f"{args.cmd}: K={k} ll={ll:.3f} iterations={it} ALS={als_it} ({dt:.2f}s) -> {base}.Q.txt")
        if cv is not None:
            cv_rows.append(dict(k=k, cverror=cv["cverror"], cverror_se=cv["cverror_se"], cv_folds=cv_folds, wall=dt + dt_cv,
                                q_out=f"{base}.Q.txt", p_npy_out=f"{base}.P.npy", p_site_out=f"{base}.P.site",
                                log_path=f"{base}.fastpop.log"))
            print(f"{args.cmd}: K={k} CVerror={cv['cverror']:.6f} (SE={cv['cverror_se']:.6f}, folds={cv_folds}) ({dt_cv:.2f}s)")
    with open(os.path.join(outdir, f"{prefix}.fastpop.summary.log"), "w") as fh:
        fh.write(f"genotype: {prefix_in}\nsamples: {sess.n_samples}\nkept SNPs: {sess.n_snps}\nK spec: {args.k}\n")
        fh.write("K\tll_final\tinit_ll\tadam_iter\tals_iter\tseconds\n")
        for k, ll, init_ll, it, als_it, dt in summary:
            fh.write(f"{k}\t{ll:.6f}\t{init_ll:.6f}\t{it}\t{als_it}\t{dt:.3f}\n")
        if cv_rows:
            best = min(cv_rows, key=lambda r: r["cverror"])
            fh.write("K\tCVerror\tSE\tCVfolds\tseconds\n")
            for r in cv_rows:
                fh.write(f"{r['k']}\t{r['cverror']:.6f}\t{r['cverror_se']:.6f}\t{r['cv_folds']}\t{r['wall']:.3f}\n")
            fh.write(f"Best K by CVerror: K={best['k']} (CVerror={best['cverror']:.6f}, SE={best['cverror_se']:.6f})\n")
        fh.write(f"total seconds: {time.perf_counter() - t0:.3f}\n")
    if cv_rows:
        tsv = os.path.join(outdir, f"{prefix}.fastpop.cverror.summary.tsv")
        write_cverror_summary_tsv(tsv, cv_rows)
        print(f"{args.cmd}: Best K by CVerror: K={best['k']} (CVerror={best['cverror']:.6f}, SE={best['cverror_se']:.6f}) -> {tsv}")
    return 0


_TREE_NJ_UNBUILT = ("bionj", "bionj-dist", "bionj-jc", "bionj-binom", "bionj-auto", "approx")


def cmd_tree(args):
    """`jx tree -bfile PREFIX -nj [exact]` (python/janusx/script/tree.py:585-720): the sites the chunk loader keeps, their DNA
    alignment, JC69 distances and the exact neighbour-joining tree -> `{out}.nwk`, `{out}.fasta` (unless --no-fasta, an extension:
    the alignment is n x sites bytes) and `{out}.phy` with --write-phylip.  The reference's `.log` and `--profile` files are not
    written; the other NJ modes, -ml and non-BED input are refused."""
    for flag, what in (("fasta", "-fa"), ("vcf", "-vcf"), ("hmp", "-hmp"), ("file", "-file")):
        if getattr(args, flag, None):
            raise SystemExit(f"tree: {what} input is not supported on this build; give a PLINK prefix with -bfile")
    if args.ml:
        raise SystemExit("tree: -ml (FastTree maximum likelihood) is not built on this build; use -nj")
    if not args.bfile:
        raise SystemExit("tree needs -bfile PREFIX")
    mode = "exact" if args.nj is None else str(args.nj).strip().lower()
    if mode in _TREE_NJ_UNBUILT:
        raise SystemExit(f"tree: -nj {mode} is not built on this build; exact neighbour joining only (-nj or -nj exact)")
    if mode != "exact":
        raise SystemExit(f"tree: unknown -nj mode '{args.nj}' (exact; the reference also has {', '.join(_TREE_NJ_UNBUILT)})")
    rank, _world = _dist_setup()
    if rank != 0:                                             # one GPU does the work
        return 0
    from . import janusx as jxrs
    src = jxrs._bed_prefix(args.bfile)
    out = _resolve_out(args, src)
    t0 = time.perf_counter()
    try:
        res = jxrs.tree_from_bed(src, args.maf, args.geno, args.het, bool(args.snps_only), out=out,
                                 write_phylip_file=bool(args.write_phylip), write_fasta_file=not args.no_fasta)
    except (RuntimeError, ValueError, OSError) as e:
        raise SystemExit(f"tree: {e}") from None
    print(f"tree: samples={len(res['sample_ids'])}, sites={res['n_sites']}, NJ mode exact, finished in "
          f"{time.perf_counter() - t0:.2f} s (the reference's .log and --profile files are not written on this build)")
    for path in res["outputs"]:
        print(f"  {path}")
    return 0


def cmd_fvlmm2(args):
    """`jx fvlmm2 -bfile PREFIX -p PHENO -i PAIRS.txt` (python/janusx/script/fvlmm2.py:887-1117): for every SNP pair of the
    interaction file the joint test of  y = covariates + SNP1 + SNP2 + combo + Zu + e  at the null model's lambda
    -> `{out}.{trait}.fvlmm2.tsv`, and `{out}.fvlmm2.skip` for the lines that did not resolve.  The pair rows are rotated with the
    trait's eigenvectors before the test (the reference's script leaves them unrotated; README, known differences).  Extensions:
    -among SNPS.txt [--op OP] tests all pairs among the named SNPs, -pmax P writes only the rows with p_combo_joint <= P,
    -screen [P] scores every pair of the active rows against every combo variant first (`fvlmm2_screen_packed`, csrc/k_pairscreen.hip)
    -> `{out}.{trait}.fvlmm2.screen.tsv`, and hands the best -screen-top hits to the joint test.  The
    reference's `.fvlmm2.log` and configuration banner are not written; non-BED input is refused."""
    from . import fvlmm2 as f2
    for flag, what in (("vcf", "-vcf"), ("hmp", "-hmp"), ("file", "-file")):
        if getattr(args, flag, None):
            raise SystemExit(f"fvlmm2: {what} input is not supported on this build; give a PLINK prefix with -bfile")
    if not args.bfile:
        raise SystemExit("fvlmm2 needs -bfile PREFIX")
    screen = getattr(args, "screen", None) is not None
    variants = t_min = None
    if screen:
        if args.interaction or args.among:
            raise SystemExit("fvlmm2: -screen finds its own pairs and cannot be combined with -i or -among (restrict its rows with "
                             "-screen-among SNPS.txt)")
        try:
            t_min = f2.chi2_1_quantile(args.screen)
            variants = f2.screen_variants(args.screen_ops)
        except ValueError as e:
            raise SystemExit(f"fvlmm2: {e}") from None
        if int(args.screen_top) < 1:
            raise SystemExit("-screen-top must be >= 1")
        if int(args.screen_min_dist) < 0:
            raise SystemExit("-screen-min-dist must be >= 0")
        if args.screen_among and not os.path.isfile(args.screen_among):
            raise SystemExit(f"fvlmm2: -screen-among file not found: {args.screen_among}")
    elif not args.interaction and not args.among:
        raise SystemExit("fvlmm2 needs an interaction file (-i PAIRS.txt) and/or -among SNPS.txt")
    if int(args.n_tests) < 0:
        raise SystemExit("--n-tests must be >= 0")
    if args.pmax is not None and not (0.0 <= float(args.pmax) <= 1.0):
        raise SystemExit("-pmax must be within [0, 1]")
    if args.op not in f2.OPS:
        raise SystemExit(f"--op must be one of {' '.join(f2.OPS)}")
    for path, what in ((args.interaction, "Interaction file"), (args.among, "-among file"), (args.pheno, "Phenotype file")):
        if path and not os.path.isfile(path):
            raise SystemExit(f"fvlmm2: {what} not found: {path}")
    among_names = None
    if args.among:
        try:
            among_names = f2.read_among_names(args.among)
        except ValueError as e:
            raise SystemExit(f"fvlmm2: {e}") from None
    rank, _world = _dist_setup()
    if rank != 0:                                             # one GPU does the work
        return 0
    import torch
    from . import janusx as jxrs
    from . import pipeline as pl
    from .bed import read_fam_ids
    src = jxrs._bed_prefix(args.bfile)
    t0 = time.perf_counter()
    # the active rows: `prepare_packed_ctx_from_plink` (filter over all samples, no flips, maf = ALT frequency), fvlmm2.py:1037-1046
    try:
        pk, _miss, maf, _std, flip, site_keep, n_fam, _total = jxrs.prepare_bed_2bit_packed(
            src, float(args.maf), float(args.geno), float(args.het), bool(args.snps_only))
    except (RuntimeError, ValueError, OSError) as e:
        raise SystemExit(f"fvlmm2: {e}") from None
    chrom, pos_bp, snp, _a0, _a1 = jxrs.load_bim_columns(src, np.nonzero(site_keep)[0])
    row_names, name_map = f2.build_name_map(chrom, pos_bp, snp)
    specs, skipped = f2.parse_interaction_file(args.interaction, name_map) if args.interaction else ([], [])
    if among_names is not None:
        sp2, sk2 = f2.among_specs(among_names, name_map, row_names, args.op)
        specs, skipped = specs + sp2, skipped + sk2
    screen_rows = None
    if screen and args.screen_among:                          # no cap on the names: the screen takes any row list
        with open(args.screen_among, "r", encoding="utf-8", errors="replace") as fh:
            wanted = [w[0] for w in (line.split() for line in fh) if w and not w[0].startswith("#")]
        found = set()
        for k, name in enumerate(wanted, start=1):
            try:
                found.add(f2.resolve_snp_token(name, name_map))
            except f2.NameLookupError as e:
                skipped.append(f2.Skipped(f"screen-among:{k}", str(name), e.reason))
        screen_rows = np.array(sorted(found), dtype=np.int64)
        if screen_rows.size < 2:
            raise SystemExit("fvlmm2: -screen-among names fewer than two active variants")
    if not specs and not screen:
        raise SystemExit(f"fvlmm2: {f2.NO_EXPRESSIONS}")
    out = _resolve_out(args, src)
    if screen:
        n_rows = len(row_names) if screen_rows is None else int(screen_rows.size)
        print(f"Screening the pairs of {n_rows} of {len(row_names)} active filtered variants, {len(variants)} variants each, "
              f"at chi2 >= {t_min:.4f} (P = {float(args.screen):g}); skipped={len(skipped)}.")
    else:
        print(f"Resolved {len(specs)} interaction rows against {len(row_names)} active filtered variants; skipped={len(skipped)}.")
    if skipped:
        f2.write_skip(f"{out}.fvlmm2.skip", skipped)
        print(f"Skipped interaction rows were written to {out}.fvlmm2.skip")
    fam = read_fam_ids(src)
    ids, names, ph = _read_table(args.pheno)
    pos = {s: i for i, s in enumerate(ids)}
    dev = torch.device("cuda", torch.cuda.current_device())
    packed_t = torch.from_numpy(pk).to(dev)
    cov_items = args.cov if isinstance(args.cov, list) else ([args.cov] if args.cov else [])
    # a `chr:pos` item of -c is looked up among the active rows of this run
    cv, cpos = _load_cov_items(cov_items, fam, types.SimpleNamespace(chrom=chrom, pos=pos_bp), packed_t, n_fam)
    if 1 + (0 if cv is None else int(cv.shape[1])) > jxrs.FVLMM2_MAX_PCOV:      # before the GRM and the eigendecomposition
        raise SystemExit(f"fvlmm2: at most {jxrs.FVLMM2_MAX_PCOV - 1} covariate columns beside the intercept on this build, got "
                         f"{int(cv.shape[1])}")
    # the GRM of `jx gwas -fvlmm` (-k FILE, else method 1 over the kept sites of this run)
    if args.grm:
        k = torch.from_numpy(_load_grm(args.grm, fam)).to(dev)
    else:
        k, eff, _ = pl.build_grm(packed_t, n_fam, 1, args.maf, args.geno)
        print(f"GRM method 1: eff_m={eff} ({time.perf_counter() - t0:.2f}s)")
    row1 = np.array([sp.row1 for sp in specs], dtype=np.int64)
    row2 = np.array([sp.row2 for sp in specs], dtype=np.int64)
    ops = [sp.op for sp in specs]
    neg1 = np.array([sp.neg1 for sp in specs], dtype=bool)
    neg2 = np.array([sp.neg2 for sp in specs], dtype=bool)
    cov_dim = 0 if cv is None else int(cv.shape[1])
    for ti in _select_traits(names, args.ncol):
        name = names[ti]
        t1 = time.perf_counter()
        keep_idx = np.array([j for j, sid in enumerate(fam)
                             if pos.get(sid) is not None and math.isfinite(ph[pos[sid], ti])
                             and (cv is None or (sid in cpos and np.all(np.isfinite(cv[cpos[sid]]))))], dtype=np.int64)
        n = len(keep_idx)
        if n <= cov_dim + 4:
            raise SystemExit(f"Trait {name} has too few usable samples after alignment/filtering: n={n}, cov={cov_dim}.")
        y = np.array([ph[pos[fam[j]], ti] for j in keep_idx])
        x = np.ones((n, 1))
        if cv is not None:
            x = np.concatenate([x, np.array([cv[cpos[fam[j]]] for j in keep_idx])], axis=1)
        model = pl.trait_null_model(k, keep_idx, x, y)
        lbd = float(model.null.lbd)
        if not (math.isfinite(lbd) and lbd > 0.0):
            raise SystemExit(f"Trait {name} produced invalid null lambda: {lbd}")
        n_tests = int(args.n_tests)
        if screen:
            # first stage: every pair of the active rows against every variant; the top K hits go on to the joint test
            resid, sigma2 = f2.screen_residual(model.S, model.xcov, model.y, model.ut, lbd)
            _names, chrom_codes = np.unique(np.asarray([str(c) for c in chrom]), return_inverse=True)
            try:
                hits = jxrs.fvlmm2_screen_packed(packed_t, n_fam, flip, resid, sigma2, variants, t_min, rows=screen_rows,
                                                 chrom_id=chrom_codes.astype(np.int32), pos=np.asarray(pos_bp, dtype=np.int64),
                                                 min_dist=int(args.screen_min_dist), sample_indices=keep_idx)
            except RuntimeError as e:
                raise SystemExit(f"fvlmm2: {e}") from None
            combo = [variants[v].spelled(row_names[a], row_names[b]) for a, b, v in zip(hits["row1"], hits["row2"], hits["variant"])]
            spath = f"{out}.{f2.trait_label(name)}.fvlmm2.screen.tsv"
            f2.write_screen_table(spath, [row_names[a] for a in hits["row1"]], [row_names[b] for b in hits["row2"]], combo,
                                  hits["n_complete"], hits["stat"])
            top = min(int(args.screen_top), len(combo))
            print(f"[{name}] screen: pairs={hits['pairs_screened']} variants={len(variants)} hits={hits['hits_total']} "
                  f"top={top} sigma2={sigma2:.5g} -> {spath}")
            specs = [f2.PairSpec(int(hits["row1"][k]), int(hits["row2"][k]), variants[hits["variant"][k]].op,
                                 variants[hits["variant"][k]].neg1, variants[hits["variant"][k]].neg2, combo[k],
                                 row_names[hits["row1"][k]], row_names[hits["row2"][k]]) for k in range(top)]
            row1 = np.array([sp.row1 for sp in specs], dtype=np.int64)
            row2 = np.array([sp.row2 for sp in specs], dtype=np.int64)
            ops = [sp.op for sp in specs]
            neg1 = np.array([sp.neg1 for sp in specs], dtype=bool)
            neg2 = np.array([sp.neg2 for sp in specs], dtype=bool)
            if n_tests == 0:                                  # every screened (pair, variant) was a hypothesis
                n_tests = int(hits["pairs_screened"]) * len(variants)
                print(f"[{name}] BH hypothesis count: {n_tests} (pairs screened x variants)")
        try:
            res = jxrs.fvlmm2_pairs_packed(packed_t, n_fam, flip, maf, row1, row2, ops, neg1, neg2, model.S, model.xcov, model.y,
                                           model.ut, math.log10(lbd), sample_indices=keep_idx, batch_size=int(args.batch_size))
        except RuntimeError as e:
            raise SystemExit(f"fvlmm2: {e}") from None
        joint = np.stack([res[c] for c in ("beta1", "se1", "p1", "beta2", "se2", "p2", "beta_combo", "se_combo", "p_combo")], axis=1)
        fdr = f2.bh_adjust(joint[:, 8], n_tests=n_tests if n_tests > 0 else None)
        keep = None if args.pmax is None else joint[:, 8] <= float(args.pmax)
        path = f"{out}.{f2.trait_label(name)}.fvlmm2.tsv"
        wrote = f2.write_table(path, [chrom[r] for r in row1], [pos_bp[r] for r in row1], [sp.expr for sp in specs],
                               res["combo_af"], joint, fdr, keep)
        print(f"[{name}] fvlmm2: n={n} pairs={len(specs)} written={wrote} lambda0={lbd:.5g} -> {path} "
              f"({time.perf_counter() - t1:.2f}s)")
        del model
    return 0


_REML_MISSING = {"", "na", "nan", "null", "none", "."}


def _read_table_text(path):
    """Header + rows of a tab/space/comma delimited table as text: (ids, column names, list of string rows)."""
    with open(path) as fh:
        header = fh.readline().rstrip("\n").replace(",", "\t").split()
        ids, rows = [], []
        for line in fh:
            parts = line.rstrip("\n").replace(",", "\t").split()
            if parts:
                ids.append(parts[0])
                rows.append(parts[1:])
    names = header[1:]
    for r in rows:
        r.extend([""] * (len(names) - len(r)))
    return ids, names, rows


def _reml_columns(spec_list):
    """The comma lists of -c / -rc as tokens; `A:B` interaction terms are not built."""
    out = []
    for spec in spec_list or []:
        for tok in str(spec).split(","):
            tok = tok.strip()
            if not tok:
                continue
            if ":" in tok:
                raise SystemExit(f"reml: the interaction term '{tok}' (A:B) is not built on this build; give single columns")
            out.append(tok)
    return out


def _reml_refusals(args):
    """Everything `jx reml` refuses is refused here, before any file is opened."""
    for flag, what in (("gxe", "-gxe"), ("gxc", "-gxc"), ("spk", "-spk"), ("spk_mode", "--spk-mode")):
        if getattr(args, flag, None):
            raise SystemExit(f"reml: {what} is not built on this build (dense multi-kernel REML over -k and -rc terms only)")
    cov, rc = _reml_columns(args.cov), _reml_columns(args.rcov)
    if not args.ncol:
        raise SystemExit("reml needs -n TRAIT")
    if not args.grm and not rc:
        raise SystemExit("reml needs at least one random term: -k GRM.npy or -rc COLUMN")
    if not args.out:
        raise SystemExit("reml needs -o OUT")
    return cov, rc


def _reml_col_index(tok, names, what):
    if tok in names:
        return names.index(tok)
    if tok.isdigit() and int(tok) < len(names):
        return int(tok)
    raise SystemExit(f"reml: unknown {what} column '{tok}'")


def cmd_reml(args):
    """`jx reml -p PHENO -n TRAIT [-k GRM.npy]... [-c COLS] [-rc COLS] -o OUT`: y = fixed + one random term per -k + one per -rc + e
    by multi-kernel AI-REML on the device (`blup.BLUP`; python/janusx/pyBLUP/blup.py:610-1004 is the class behind the reference's
    `jx reml`).  Samples: the ids present in every -k id list with the trait, every -c and every -rc column non-missing, in
    phenotype order; each id once.  -> `{out}.reml.vc.tsv` (trait, n, term, theta, var, pve, reml, ml, iters, route; one line per
    term, residual last) and `{out}.reml.blup.tsv` (id, trait, fixed, one column per random term, residual).  These tables are this
    build's own: the reference's `.reml.summary.tsv`, `.blue.txt`, `.blup.txt` belong to its line x environment workflow, which is
    refused (a repeated id), as are -gxe, -gxc, -spk, --spk-mode, A:B terms and non-numeric -c columns.  -exact-trace is an
    extension: the exact trace of V^-1 K_j at every n (the reference uses Hutchinson probes above n = 768)."""
    cov_tok, rc_tok = _reml_refusals(args)
    rank, _world = _dist_setup()
    if rank != 0:                                             # one GPU does the work
        return 0
    ids, names, rows = _read_table_text(args.pheno)
    seen = set()
    for s in ids:
        if s in seen:
            raise SystemExit(f"reml: sample id '{s}' occurs more than once in {args.pheno}; repeated records per line are the "
                             "reference's line x environment workflow, which is not built on this build")
        seen.add(s)
    traits = _select_traits(names, args.ncol)
    cov_idx = [_reml_col_index(t, names, "-c") for t in cov_tok]
    rc_idx = [_reml_col_index(t, names, "-rc") for t in rc_tok]

    def missing(v):
        return v.strip().lower() in _REML_MISSING

    def number(v, col):
        try:
            return float(v)
        except ValueError:
            raise SystemExit(f"reml: -c column '{names[col]}' is not numeric ('{v}'); categorical fixed effects are not built "
                             "on this build, give the column to -rc") from None

    cov_val = np.full((len(ids), len(cov_idx)), np.nan)
    for j, c in enumerate(cov_idx):
        for i, r in enumerate(rows):
            if not missing(r[c]):
                cov_val[i, j] = number(r[c], c)
    grm_ids = []
    for path in args.grm or []:
        id_path = path + ".id"
        if os.path.exists(id_path):
            with open(id_path) as fh:
                grm_ids.append([ln.split()[0] for ln in fh if ln.strip()])
        else:
            grm_ids.append(list(ids))                          # no id file: the matrix is in phenotype order (_load_grm checks its shape)
    grm_sets = [set(g) for g in grm_ids]
    in_all = [all(s in g for g in grm_sets) for s in ids]
    # every matrix is loaded once, over the records present in all of them (phenotype order); a trait takes its rows from that
    common = [i for i in range(len(ids)) if in_all[i]]
    common_pos = {i: k for k, i in enumerate(common)}
    grm_common = []
    for path in args.grm or []:
        if os.path.exists(path + ".id"):
            grm_common.append(np.asarray(_load_grm(path, [ids[i] for i in common]), dtype=np.float64))
        else:
            grm_common.append(np.asarray(_load_grm(path, ids), dtype=np.float64)[np.ix_(common, common)])
    from . import blup
    out = args.out
    parent = os.path.dirname(out)
    if parent:
        os.makedirs(parent, exist_ok=True)
    vc_lines, blup_lines = [], []
    terms = [f"rc:{names[c]}" for c in rc_idx] + [f"k:{os.path.basename(p)}" for p in args.grm or []]
    for t in traits:
        keep = []
        for i, r in enumerate(rows):
            if not in_all[i] or missing(r[t]) or any(missing(r[c]) for c in rc_idx) or not np.all(np.isfinite(cov_val[i])):
                continue
            try:
                float(r[t])
            except ValueError:
                continue
            keep.append(i)
        if len(keep) < 3:
            raise SystemExit(f"reml: trait '{names[t]}' has {len(keep)} usable samples")
        sel_ids = [ids[i] for i in keep]
        y = np.array([float(rows[i][t]) for i in keep])
        x = cov_val[keep] if cov_idx else None
        z_list = []
        for c in rc_idx:
            levels = sorted({rows[i][c] for i in keep})
            pos = {v: k for k, v in enumerate(levels)}
            z = np.zeros((len(keep), len(levels)))
            z[np.arange(len(keep)), [pos[rows[i][c]] for i in keep]] = 1.0
            z_list.append(z)
        sub = [common_pos[i] for i in keep]
        g_list = [np.ascontiguousarray(g[np.ix_(sub, sub)]) for g in grm_common]
        t0 = time.perf_counter()
        try:
            fit = blup.BLUP(y, X=x, Z=z_list or None, G=g_list or None, maxiter=args.maxiter, progress=False,
                            exact_trace=bool(args.exact_trace))
        except (RuntimeError, ValueError, np.linalg.LinAlgError) as e:
            raise SystemExit(f"reml: {e}") from None
        total = float(np.sum(fit.var))
        for term, th, v in zip(terms + ["residual"], fit.theta, fit.var):
            vc_lines.append(f"{names[t]}\t{len(keep)}\t{term}\t{th:.10g}\t{v:.10g}\t{v / total:.10g}\t{fit.reml:.10g}\t{fit.ml:.10g}\t"
                            f"{int(getattr(fit.result, 'nit', 0))}\t{fit.route}")
        fixed = fit.X @ fit.beta
        parts, start = [], 0
        for z, w in zip(z_list, fit.z_cols):
            parts.append(z @ fit.u[start:start + w])
            start += w
        parts += list(fit.g_by_G)
        for k, s in enumerate(sel_ids):
            cells = "\t".join(f"{float(pt[k, 0]):.10g}" for pt in parts)
            blup_lines.append(f"{s}\t{names[t]}\t{float(fixed[k, 0]):.10g}\t{cells}\t{float(fit.residuals[k, 0]):.10g}")
        print(f"reml: trait {names[t]}: n={len(keep)}, route {fit.route}, {int(getattr(fit.result, 'nit', 0))} iterations, "
              f"reml={fit.reml:.6f}, pve " + ", ".join(f"{tm}={v / total:.4f}" for tm, v in zip(terms, fit.var))
              + f" ({time.perf_counter() - t0:.2f} s)")
    with open(out + ".reml.vc.tsv", "w") as fh:
        fh.write("trait\tn\tterm\ttheta\tvar\tpve\treml\tml\titers\troute\n" + "".join(ln + "\n" for ln in vc_lines))
    with open(out + ".reml.blup.tsv", "w") as fh:
        fh.write("id\ttrait\tfixed\t" + "\t".join(terms) + "\tresidual\n" + "".join(ln + "\n" for ln in blup_lines))
    print(f"  {out}.reml.vc.tsv\n  {out}.reml.blup.tsv")
    return 0


def _add_admixture_parser(sub, name):
    a = sub.add_parser(name)
    a.add_argument("-bfile", "--bfile", default=None)
    a.add_argument("-vcf", "--vcf", default=None, help=argparse.SUPPRESS)
    a.add_argument("-hmp", "--hmp", default=None, help=argparse.SUPPRESS)
    a.add_argument("-file", "--file", default=None, help=argparse.SUPPRESS)
    a.add_argument("-k", "--k", type=str, required=True,
                   help="K spec: single (8), range (1..10 or 1:10), stepped range (1..10..3, 1:10:3, or 1..10:3), or list (1,5,8)")
    a.add_argument("-o", "--out", default=None, help="output directory (default: current directory)")
    a.add_argument("-prefix", "--prefix", default=None, help="output file prefix (default: the genotype basename)")
    a.add_argument("-maf", "--maf", type=float, default=0.02)
    a.add_argument("-geno", "--geno", type=float, default=0.05)
    a.add_argument("-snps-only", "--snps-only", dest="snps_only", action="store_true", default=False,
                   help="drop sites whose alleles are not single A/C/G/T")
    a.add_argument("-seed", "--seed", type=int, default=42)
    a.add_argument("-solver", "--solver", type=str, default="adam-em", choices=["auto", "adam", "adam-em"])
    a.add_argument("-max-iter", "--max-iter", dest="max_iter", type=int, default=500)
    a.add_argument("-check", "--check", type=int, default=5)
    a.add_argument("-tol", "--tol", type=float, default=1e-5)
    a.add_argument("-cv", "--cv", type=int, default=None, help="the reference's spelling: refused for N >= 2, see -cverror")
    a.add_argument("-cverror", "--cverror", type=int, nargs="?", const=5, default=None, metavar="N",
                   help="choose K by N-fold cross-validation error (bare: 5 folds; 2 <= N <= 256; 0 = off)")
    a.add_argument("--no-plot", dest="no_plot", action="store_true", default=False, help="accepted; plots are never drawn")
    a.add_argument("-tag", "--tag", default=None, help="accepted and unused (plots are not built)")
    a.add_argument("-t", "--thread", "-threads", "--threads", dest="thread", type=int, default=None,
                   help="accepted for compatibility; unused")
    a.add_argument("-mem", "--memory", dest="memory", type=float, default=None, help="accepted for compatibility; unused")
    a.set_defaults(func=cmd_adamixture)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="jx", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    g = sub.add_parser("gwas")
    g.add_argument("-bfile", "--bfile", required=True)
    g.add_argument("-p", "--pheno", required=True)
    g.add_argument("-n", "--n", dest="ncol", action="append", default=None)
    g.add_argument("-lm", "--lm", action="store_true", default=False,
                   help="plain linear model -> {out}.{trait}.lm.tsv")
    g.add_argument("-trait-level", "--trait-level", dest="trait_level", action="store_true", default=False,
                   help="with -lm and two or more traits: traits that share a sample mask are scanned together on the matrix "
                        "pipes and all land in one table {out}.lm.tsv with a phenotype column")
    g.add_argument("-trait-level-lmm", "--trait-level-lmm", dest="trait_level_lmm", action="store_true", default=False,
                   help="with -lmm and two or more traits: traits that share a sample mask share one eigendecomposition and one "
                        "rotation of every SNP block and all land in one table {out}.lmm.tsv with a phenotype column")
    g.add_argument("-trait-pmax", "--trait-pmax", dest="trait_pmax", type=float, default=None, metavar="P",
                   help="with -trait-level / -trait-level-lmm: write only the rows with pwald <= P (an extension; the reference "
                        "has no such flag)")
    g.add_argument("-lm2", "--lm2", nargs="?", const="__SELF__", default=None, metavar="COVCOL",
                   help="linear model with SNP-by-covariate interaction terms over the selected columns of the merged -c table "
                        "-> {out}.{trait}.lm2.tsv; 0-based selectors like 0, 0:3, :2, 0,3; without columns it runs -lm")
    g.add_argument("-farmcpu", "--farmcpu", dest="farmcpu", action="store_true", default=False,
                   help="FarmCPU, the classic (raw) route -> {out}.{trait}.farmcpu.tsv and, when pseudo-QTNs exist, "
                        "{out}.{trait}.farmcpu.qtn")
    g.add_argument("-frgwas", "--frgwas", dest="frgwas", action="store_true", default=False, help=argparse.SUPPRESS)
    g.add_argument("-algwas", "--algwas", dest="algwas", action="store_true", default=False, help=argparse.SUPPRESS)
    g.add_argument("--farmcpu-iter", dest="farmcpu_iter", type=int, default=30, help="FarmCPU iteration cap (default 30)")
    g.add_argument("--farmcpu-threshold", dest="farmcpu_threshold", type=float, default=None,
                   help="FarmCPU p threshold (default 1 / tested SNP count)")
    g.add_argument("--farmcpu-qtn-bound", dest="farmcpu_qtn_bound", type=str, default="auto",
                   help="largest lead count of the FarmCPU lead search (default auto = floor(sqrt(n / log10 n)))")
    g.add_argument("--farmcpu-nbin", dest="farmcpu_nbin", type=int, default=5, help="lead-count grid size (default 5)")
    g.add_argument("--farmcpu-bin-size", dest="farmcpu_bin_size", type=str, default="500000,5000000,50000000",
                   help="comma-separated bin sizes in bp (default 500000,5000000,50000000)")
    g.add_argument("-lmm", "--lmm", action="store_true", default=False)
    g.add_argument("-lmm2", "--lmm2", action="store_true", default=False)
    g.add_argument("-fvlmm", "--fvlmm", action="store_true", default=False)
    g.add_argument("-k", "--grm", dest="grm", type=str, default="1")
    g.add_argument("-c", "--cov", dest="cov", action="append", default=None,
                   help="covariate table (sample id + columns) or a SNP site chr:pos taken as a covariate; may be repeated")
    g.add_argument("-snps-only", "--snps-only", dest="snps_only", action="store_true", default=False,
                   help="drop sites whose alleles are not single A/C/G/T")
    g.add_argument("-mem", "--memory", dest="memory", type=float, default=None,
                   help="accepted for compatibility; unused (the working set lives in HBM)")
    g.add_argument("-v", "--verbose", action="store_true", default=False, help="accepted for compatibility")
    g.add_argument("-q", "--qcov", dest="qcov", type=str, default="0",
                   help="number of principal components of the GRM added as covariates (integer >= 0; external covariates "
                        "go through -c)")
    g.add_argument("-mmap-window-mb", "--mmap-window-mb", dest="mmap_window_mb", type=int, default=None,
                   help="stage the .bed payload to the device in windows of this many MiB (default 256)")
    g.add_argument("-maf", "--maf", type=float, default=0.02)
    g.add_argument("-geno", "--geno", type=float, default=0.05)
    g.add_argument("-het", "--het", type=float, default=1.0)
    g.add_argument("-o", "--out", default=None)
    g.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    g.add_argument("-force-model", "--force-model", dest="force_model", action="store_true", default=False)
    g.add_argument("-chunksize", "--chunksize", dest="chunksize", type=int, default=10000,
                   help="SNP rows per scan chunk (the reference's default 10000): the length of a warm-start chain of -lmm")
    g.add_argument("-warm-start", "--warm-start", dest="warm_start", choices=["chain", "none"], default=None,
                   help="-lmm: 'chain' (the reference's default: each SNP's Brent starts from the previous SNP's optimum inside "
                        "a chunk) or 'none'; default chain unless JX_LMM_UNIFIED_NO_WARM_START is set")
    g.add_argument("-warm-chain-pieces", "--warm-chain-pieces", dest="warm_chain_pieces", type=int, default=1,
                   help="cut every chunk's chain into this many pieces (power of two) by halving, as rayon's splitter does on "
                        "the reference's thread pool (2 x threads pieces); 1 = one chain per chunk")
    g.add_argument("-t", "--thread", type=int, default=0, help="accepted for compatibility; unused")
    g.set_defaults(func=cmd_gwas)
    g.add_argument("-splmm", "--splmm", "-splmm-approx", "--splmm-approx", dest="splmm", nargs="?", const=0.05, default=None,
                   type=float,
                   help="SparseLMM with the GRAMMAR-gamma scan approximation (fastGWA null + residualised scan) on a sparse GRM "
                        "thresholded at this kinship cut-off (default 0.05; negative: keep every entry); -k FILE.spgrm reuses "
                        "an existing sparse GRM")
    g.add_argument("-spk", "--grm-sparse", dest="grm_sparse", type=str, default="1",
                   help="sparse GRM of the SparseLMM models: 1 (centering), 2 (standardization) or a precomputed .spgrm / .jxgrm "
                        "file with its .id sibling")
    g.add_argument("-splmm-exact", "--splmm-exact", dest="splmm_exact", nargs="?", const=0.05, default=None, type=float,
                   help="SparseLMM with the exact g'Pg denominator for every SNP -> {out}.{trait}.splmm2.tsv")
    r = sub.add_parser("grm")
    r.add_argument("-bfile", "--bfile", default=None)
    r.add_argument("-m", "--method", type=int, default=1, choices=[1, 2])
    r.add_argument("-maf", "--maf", type=float, default=0.02)
    r.add_argument("-geno", "--geno", type=float, default=0.05)
    r.add_argument("-o", "--out", default=None)
    r.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    r.add_argument("-grm", "--grm", "-k", "--dense-grm", dest="grm", default=None,
                   help="existing dense GRM (.npy with a sibling .id); with -sparse it is thresholded into a .spgrm "
                        "(-k / --dense-grm is the reference's name of this option)")
    r.add_argument("-snps-only", "--snps-only", dest="snps_only", action="store_true", default=False,
                   help="drop sites whose alleles are not single A/C/G/T")
    r.add_argument("-mem", "--memory", dest="memory", type=float, default=None, help="accepted for compatibility; unused")
    r.add_argument("-v", "--verbose", action="store_true", default=False, help="accepted for compatibility")
    r.add_argument("-txt", "--txt", action="store_true", default=False,
                   help="write the dense GRM as plain text ({out}.cGRM.txt, %%.6f) instead of NPY")
    r.add_argument("-sparse", "--sparse", nargs="?", const=0.05, default=None, type=float,
                   help="write a sparse `.spgrm` keeping off-diagonal kinship > cutoff (negative: keep everything)")
    r.add_argument("-king", "--king", nargs="?", const=0.05, default=None, type=float,
                   help="KING robust kinship instead of a GRM (an extension: the reference has the function and no command): "
                        "related pairs with kinship >= THRESHOLD (bare flag: 0.05) -> {out}.king.kin0, the greedy unrelated set -> "
                        "{out}.king.unrelated.id and the removed samples -> {out}.king.related.id.  Sites are filtered by this "
                        "command's -maf / -geno defaults (0.02 / 0.05), not the function's (0.01 / 0.1); not with -sparse / -grm / -txt")
    r.add_argument("-t", "--thread", type=int, default=0, help="accepted for compatibility; unused")
    r.set_defaults(func=cmd_grm)
    q = sub.add_parser("gs")
    q.add_argument("-bfile", "--bfile", required=True)
    q.add_argument("-p", "--pheno", required=True)
    q.add_argument("-n", "--n", dest="ncol", action="append", default=None)
    q.add_argument("-BLUP", "--BLUP", dest="blup", action="store_true", default=False)
    q.add_argument("-GBLUP", "--GBLUP", dest="gblup", action="store_true", default=False)
    q.add_argument("-rrBLUP", "--rrBLUP", dest="rrblup", action="store_true", default=False)
    q.add_argument("-rr-solver", "--rr-solver", "--rrblup-solver", dest="rr_solver", choices=["auto", "exact", "fast", "pcg"], default="auto",
                   help="rrBLUP: exact marker-space route (auto up to 15000 kept markers) or PCG")
    q.add_argument("-lambda", "--lambda", "--rrblup-lambda", dest="lam", type=float, default=None)
    q.add_argument("-lambda-reml", "--lambda-reml", dest="lambda_reml", action="store_true", default=False,
                   help="rrBLUP: take lambda from the subsample GBLUP REML instead of Haseman-Elston")
    q.add_argument("-tol", "--tol", type=float, default=1e-4)
    q.add_argument("-max-iter", "--max-iter", dest="max_iter", type=int, default=100)
    q.add_argument("-cv", "--cv", type=int, default=None)
    q.add_argument("-seed", "--seed", type=int, default=42)
    q.add_argument("-k", "--grm", dest="grm", type=str, default=None)
    q.add_argument("-maf", "--maf", type=float, default=0.02)
    q.add_argument("-geno", "--geno", type=float, default=0.05)
    q.add_argument("-o", "--out", default=None)
    q.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    q.add_argument("-t", "--thread", type=int, default=0, help="accepted for compatibility; unused")
    q.set_defaults(func=cmd_gs)
    c = sub.add_parser("pca")
    c.add_argument("-bfile", "--bfile", default=None)
    c.add_argument("-k", "--grm", dest="grm", default=None,
                   help="GRM file or prefix (.cGRM.npy / .sGRM.npy / .grm.npy / .txt with a sibling .id)")
    c.add_argument("-vcf", "--vcf", default=None, help=argparse.SUPPRESS)
    c.add_argument("-hmp", "--hmp", default=None, help=argparse.SUPPRESS)
    c.add_argument("-file", "--file", default=None, help=argparse.SUPPRESS)
    c.add_argument("-dim", "--dim", type=int, default=3)
    c.add_argument("-maf", "--maf", type=float, default=0.02)
    c.add_argument("-geno", "--geno", type=float, default=0.05)
    c.add_argument("-rsvd", "--rsvd", nargs="*", default=None, metavar="RSVD_ARG",
                   help="randomized SVD of the genotypes: '-rsvd', '-rsvd 3' or '-rsvd 3 0.1' (power, tol; seed 42)")
    c.add_argument("-snps-only", "--snps-only", dest="snps_only", action="store_true", default=False,
                   help="drop sites whose alleles are not single A/C/G/T")
    c.add_argument("-c", "--qcov", dest="qcov", default=None, help=argparse.SUPPRESS)
    c.add_argument("-plot", "--plot", dest="plot", action="store_true", default=False, help=argparse.SUPPRESS)
    c.add_argument("-plot3D", "--plot3D", dest="plot3d", action="store_true", default=False, help=argparse.SUPPRESS)
    c.add_argument("-group", "--group", dest="group", default=None, help=argparse.SUPPRESS)
    c.add_argument("-palette", "--palette", dest="palette", default=None, help=argparse.SUPPRESS)
    c.add_argument("-o", "--out", default=None)
    c.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    c.add_argument("-mem", "--memory", dest="memory", type=float, default=None, help="accepted for compatibility; unused")
    c.add_argument("-v", "--verbose", action="store_true", default=False, help="accepted for compatibility")
    c.add_argument("-t", "--thread", type=int, default=0, help="accepted for compatibility; unused")
    c.set_defaults(func=cmd_pca)
    _add_admixture_parser(sub, "adamixture")
    _add_admixture_parser(sub, "fastpop")
    f = sub.add_parser("gformat")
    f.add_argument("-bfile", "--bfile", default=None)
    f.add_argument("-prune", "--prune", nargs=3, default=None, metavar=("WINDOW", "STEP", "R2"),
                   help="LD prune with MAF priority: window (variant count, or with a kb / bp suffix), step (variants), r^2")
    f.add_argument("-o", "--out", default=None)
    f.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    f.add_argument("-t", "--thread", "--threads", dest="thread", type=int, default=0, help="accepted for compatibility; unused")
    for flag in ("vcf", "hmp", "file", "keep", "extract", "snp-name", "chr"):
        f.add_argument(f"-{flag}", f"--{flag}", dest=flag.replace("-", "_"), default=None, help=argparse.SUPPRESS)
    f.add_argument("-fmt", "--fmt", dest="format", default=None, help=argparse.SUPPRESS)
    for flag in ("maf", "geno", "het"):
        f.add_argument(f"-{flag}", f"--{flag}", type=float, default=None, help=argparse.SUPPRESS)
    for flag in ("from-bp", "to-bp"):
        f.add_argument(f"-{flag}", f"--{flag}", dest=flag.replace("-", "_"), type=int, default=None, help=argparse.SUPPRESS)
    for flag in ("snps-only", "biallelic-only"):
        f.add_argument(f"-{flag}", f"--{flag}", dest=flag.replace("-", "_"), action="store_true", default=False,
                       help=argparse.SUPPRESS)
    f.set_defaults(func=cmd_gformat)
    g = sub.add_parser("gstats")
    g.add_argument("-bfile", "--bfile", default=None)
    g.add_argument("-freq", "--freq", action="store_true", default=False, help="site MAF table {out}.freq")
    g.add_argument("-miss", "--miss", action="store_true", default=False, help="missing-rate tables {out}.imiss / {out}.lmiss")
    g.add_argument("-het", "--het", action="store_true", default=False, help="heterozygosity tables {out}.ihet / {out}.lhet")
    g.add_argument("-ldsc", "--ldsc", nargs="?", const="100kb", default=None, metavar="WINDOW",
                   help="LD scores {out}.{N}.{window}.ldsc; WINDOW: SNP count (100), 100kb / 0.1mb / 100000b, or 10cm; default 100kb")
    g.add_argument("-o", "--out", default=None)
    g.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    g.add_argument("-t", "--thread", "--threads", dest="thread", type=int, default=0, help="accepted for compatibility; unused")
    for flag in ("vcf", "hmp", "file"):
        g.add_argument(f"-{flag}", f"--{flag}", dest=flag, default=None, help=argparse.SUPPRESS)
    g.set_defaults(func=cmd_gstats)
    t = sub.add_parser("tree")
    t.add_argument("-bfile", "--bfile", default=None)
    t.add_argument("-nj", "--nj", nargs="?", const="exact", default=None, metavar="MODE",
                   help="neighbour joining (the default workflow); MODE: exact (the only one built)")
    t.add_argument("-ml", "--ml", action="store_true", default=False, help=argparse.SUPPRESS)
    t.add_argument("-maf", "--maf", type=float, default=0.02)
    t.add_argument("-geno", "--geno", type=float, default=0.05)
    t.add_argument("-het", "--het", type=float, default=0.02)
    t.add_argument("-snps-only", "--snps-only", dest="snps_only", action="store_true", default=False,
                   help="drop sites whose alleles are not single A/C/G/T")
    t.add_argument("-o", "--out", default=None)
    t.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    t.add_argument("--write-phylip", dest="write_phylip", action="store_true", default=False,
                   help="also write the relaxed PHYLIP alignment {out}.phy")
    t.add_argument("--no-fasta", dest="no_fasta", action="store_true", default=False,
                   help="do not write {out}.fasta (an extension: the alignment is samples x sites bytes)")
    t.add_argument("-chunksize", "--chunksize", dest="chunksize", type=int, default=10000, help="accepted for compatibility; unused")
    t.add_argument("-t", "--thread", "--threads", dest="thread", type=int, default=0, help="accepted for compatibility; unused")
    for flag in ("fa", "vcf", "hmp", "file"):
        t.add_argument(f"-{flag}", *(("--fasta",) if flag == "fa" else (f"--{flag}",)), dest="fasta" if flag == "fa" else flag,
                       default=None, help=argparse.SUPPRESS)
    t.set_defaults(func=cmd_tree)
    v = sub.add_parser("fvlmm2")
    v.add_argument("-bfile", "--bfile", default=None)
    v.add_argument("-p", "--pheno", required=True)
    v.add_argument("-n", "--n", dest="ncol", action="append", default=None)
    v.add_argument("-i", "--interaction", dest="interaction", default=None,
                   help="interaction file, one expression per line: snp1*snp2, snp1&snp2, snp1|snp2, snp1^snp2; '!' negates a "
                        "literal of the logic operators")
    v.add_argument("-among", "--among", dest="among", default=None, metavar="SNPS.txt",
                   help="test all unordered pairs among the SNPs named in this file, one name per line, at most 4096 (an "
                        "extension); may be combined with -i, whose rows come first")
    v.add_argument("--op", dest="op", default="*", help="operator of the -among pairs: *, &, | or ^ (default *)")
    v.add_argument("-screen", "--screen", dest="screen", type=float, nargs="?", const=1e-5, default=None, metavar="P",
                   help="exhaustive first stage (an extension): score every pair of the active rows against every combo variant on "
                        "the int8 pipes, keep the hits whose chi2_1 p-value is <= P (default 1e-5) in "
                        "{out}.{trait}.fvlmm2.screen.tsv and hand the best -screen-top of them to the joint test.  p_screen ranks, "
                        "it does not test: it uses the samples called at both SNPs (the joint test imputes), hard calls for '*', "
                        "and the GRAMMAR residual of the null fit with one global variance.  Not with -i or -among")
    v.add_argument("-screen-top", "--screen-top", dest="screen_top", type=int, default=4096, metavar="K",
                   help="hits handed to the joint test (default 4096, one device batch)")
    v.add_argument("-screen-ops", "--screen-ops", dest="screen_ops", default="*,&,|,^", metavar="SPEC",
                   help="comma-separated operators of the screen; '&' and '|' stand for their four negation patterns, '!&', '&!', "
                        "'!&!' for one (default '*,&,|,^': 10 variants; at most 16)")
    v.add_argument("-screen-min-dist", "--screen-min-dist", dest="screen_min_dist", type=int, default=0, metavar="BP",
                   help="do not screen pairs on one chromosome closer than BP (default 0: off)")
    v.add_argument("-screen-among", "--screen-among", dest="screen_among", default=None, metavar="SNPS.txt",
                   help="screen only the pairs among the SNPs named in this file, one name per line, any number")
    v.add_argument("-pmax", "--pmax", dest="pmax", type=float, default=None, metavar="P",
                   help="write only the rows with p_combo_joint <= P (an extension); the FDR column is computed over every "
                        "tested row first")
    v.add_argument("-c", "--cov", dest="cov", action="append", default=None, help="covariate table (sample id + columns); may be repeated")
    v.add_argument("-k", "--grm", dest="grm", default=None, help="dense GRM (.npy with a sibling .id); default: built from the genotypes")
    v.add_argument("-maf", "--maf", type=float, default=0.02)
    v.add_argument("-geno", "--geno", type=float, default=0.05)
    v.add_argument("-het", "--het", type=float, default=1.0)
    v.add_argument("-snps-only", "--snps-only", dest="snps_only", action="store_true", default=False,
                   help="drop sites whose alleles are not single A/C/G/T")
    v.add_argument("--batch-size", dest="batch_size", type=int, default=4096, help="pairs per device batch")
    v.add_argument("--n-tests", dest="n_tests", type=int, default=0,
                   help="total hypothesis count of the BH adjustment of p_combo_joint (default: the tested rows)")
    v.add_argument("-o", "--out", default=None)
    v.add_argument("-prefix", "--prefix", default=None, help="file name prefix inside the -o directory")
    v.add_argument("-t", "--thread", "--threads", dest="thread", type=int, default=0, help="accepted for compatibility; unused")
    for flag in ("vcf", "hmp", "file"):
        v.add_argument(f"-{flag}", f"--{flag}", dest=flag, default=None, help=argparse.SUPPRESS)
    v.set_defaults(func=cmd_fvlmm2)
    m = sub.add_parser("reml")
    m.add_argument("-p", "--pheno", required=True)
    m.add_argument("-n", "--n", dest="ncol", action="append", default=None)
    m.add_argument("-k", "--grm", dest="grm", action="append", default=None,
                   help="dense GRM (.npy with a sibling .id); may be repeated: one variance component each")
    m.add_argument("-c", "--cov", dest="cov", action="append", default=None,
                   help="numeric fixed-effect columns of the phenotype table, by name or 0-based index, comma lists")
    m.add_argument("-rc", "--rcov", dest="rcov", action="append", default=None,
                   help="random-effect columns of the phenotype table: the distinct values of a column are its levels")
    m.add_argument("-maxiter", "--maxiter", dest="maxiter", type=int, default=100)
    m.add_argument("-exact-trace", "--exact-trace", dest="exact_trace", action="store_true", default=False,
                   help="exact trace of V^-1 K at every n (an extension; the reference uses Hutchinson probes above n = 768)")
    m.add_argument("-o", "--out", default=None)
    m.add_argument("-t", "--thread", "--threads", dest="thread", type=int, default=0, help="accepted for compatibility; unused")
    m.add_argument("-gxe", "--gxe", dest="gxe", nargs="?", const=True, default=None, help=argparse.SUPPRESS)
    m.add_argument("-gxc", "--gxc", dest="gxc", nargs="?", const=True, default=None, help=argparse.SUPPRESS)
    m.add_argument("-spk", "--spk", dest="spk", nargs="?", const=True, default=None, help=argparse.SUPPRESS)
    m.add_argument("--spk-mode", dest="spk_mode", default=None, help=argparse.SUPPRESS)
    m.set_defaults(func=cmd_reml)
    args = ap.parse_args(argv)
    return args.func(args)


if __name__ == "__main__":
    sys.exit(main())
