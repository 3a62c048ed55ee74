"""`gbrs` command line for the MI355X subcommands: same flags, defaults and log-and-continue
error behaviour as gbrs/commands.py:108-183 (`quantify`) and :153-183 (`reconstruct`).  argparse
instead of Typer so the GPU box needs nothing beyond the standard library."""
from __future__ import annotations

import argparse
import logging
import os
import sys


def configure_logging(verbose: int):
    """WARNING by default, level 19 with -v, DEBUG with -vv (utils.py:83-88)."""
    logger = logging.getLogger('gbrs')
    if not logger.handlers:
        h = logging.StreamHandler()
        h.setFormatter(logging.Formatter('[gbrs] %(message)s' if not os.getenv('GBRS_APP_DEBUG')
                                         else '[gbrs debug] %(levelname)s %(pathname)s:%(lineno)d %(message)s'))
        logger.addHandler(h)
    logger.setLevel(logging.WARNING if verbose == 0 else (19 if verbose == 1 else logging.DEBUG))
    return logger


def _existing(path):
    if not os.path.isfile(path):
        raise argparse.ArgumentTypeError(f"File '{path}' does not exist.")
    return os.path.realpath(path)


def _existing_or_list(path):
    """One file is checked here, like every other input; a comma list is split and checked by the command."""
    return path if ',' in path else _existing(path)


def build_parser():
    ap = argparse.ArgumentParser(prog='gbrs', description='GBRS numeric core on AMD MI355X')
    sub = ap.add_subparsers(dest='command', required=True)
    q = sub.add_parser('quantify', help='quantify allele-specific expressions')
    q.add_argument('-i', '--alignment-file', required=True, type=_existing)
    q.add_argument('-g', '--group-file', type=_existing, default=None)
    q.add_argument('-L', '--length-file', type=_existing, default=None)
    q.add_argument('-G', '--genotype', dest='genotype_file', type=_existing, default=None)
    q.add_argument('-o', '--outbase', default='gbrs.quantified')
    q.add_argument('-M', '--multiread-model', type=int, default=4)
    q.add_argument('-p', '--pseudocount', type=float, default=0.0)
    q.add_argument('-m', '--max-iters', type=int, default=999)
    q.add_argument('-t', '--tolerance', type=float, default=0.0001)
    q.add_argument('-a', '--report-alignment-counts', action='store_true')
    q.add_argument('-w', '--report-posterior', action='store_true',
                   help='write <outbase>.posterior.h5.  As in the reference the file holds the alignment structure '
                        'alone (incidence_only), no posterior values: see --posterior-values')
    q.add_argument('--posterior-values', action='store_true',
                   help='(extension, implies -w) <outbase>.posterior.h5 carries the read-level posterior of every stored '
                        'alignment in the last E-step as /h*/data, computed on the device')
    q.add_argument('--bootstrap', type=int, default=None, metavar='B',
                   help='(extension) after the ordinary run, B >= 2 bootstrap refits on reads resampled on the device; '
                        'writes <outbase>.isoforms.bootstrap.npz and, with a group file, <outbase>.genes.bootstrap.npz '
                        '(means and standard deviations of TPM and expected read counts)')
    q.add_argument('--bootstrap-seed', type=int, default=0, metavar='S', help='with --bootstrap: seed of the draw (default 0)')
    q.add_argument('--keep-replicates', action='store_true',
                   help='with --bootstrap: the files also carry tpm and expected_read_counts of every replicate (B x H x n)')
    q.add_argument('-v', '--verbose', action='count', default=0)
    q.add_argument('--device', type=int, default=0, help='HIP device ordinal (extension)')
    q.add_argument('--merge-identical-rows', action='store_true',
                   help='merge identical reads into weighted rows on the device (extension)')
    q.add_argument('--gpus', type=int, default=None,
                   help='shard the reads over N ranks, one process per GPU (extension; gbrs_amd/sharded.py)')
    q.add_argument('--devices', default=None,
                   help='with --gpus N: N comma-separated device ordinals (default --device + rank)')
    q.add_argument('--dist-backend', choices=('nccl', 'gloo'), default='nccl',
                   help='with --gpus: collective backend, nccl = RCCL (default); gloo allows two ranks on one GPU')
    r = sub.add_parser('reconstruct', help='reconstruct the genome based upon gene-level TPM quantities')
    samples = r.add_mutually_exclusive_group(required=True)
    samples.add_argument('-e', '--expr-file', dest='expression_file', type=_existing, default=None)
    samples.add_argument('--sample-file', type=_existing, default=None,
                         help='(extension, instead of -e) a cohort: tab separated lines `genes.tpm<TAB>outbase`, blank and '
                              '# lines skipped; the samples go through the device in launches of --batch-size')
    r.add_argument('--batch-size', type=int, default=64, help='with --sample-file: samples per device launch (default 64)')
    r.add_argument('--grid-file', type=_existing, default=None,
                   help='(extension) marker grid: also write <outbase>.interpolated.genoprobs.tsv, the founder dosages '
                        '`gbrs export` writes after `gbrs interpolate`, from the posteriors on the device')
    r.add_argument('--grid-genoprobs', action='store_true',
                   help='with --grid-file: also write <outbase>.interpolated.genoprobs.npz, the file of `gbrs interpolate`')
    r.add_argument('--sim-geno', type=int, default=None, metavar='K',
                   help='(extension) K >= 1 diplotype paths per chromosome drawn from the joint posterior on the device: '
                        'writes <outbase>.sim_geno.npz (state indices, K x genes per chromosome) and '
                        '<outbase>.sim_geno.crossovers.tsv (founder changes of the draws beside the Viterbi path\'s)')
    r.add_argument('--sim-geno-seed', type=int, default=0, metavar='S', help='with --sim-geno: seed of the draws (default 0)')
    r.add_argument('--diagnostics', action='store_true',
                   help='(extension) writes <outbase>.diagnostics.npz (per gene interval the expected founder changes and the '
                        'probability of a diplotype change, per gene the error LOD and the most likely diplotype) and '
                        '<outbase>.diagnostics.tsv (a summary per chromosome), from the posteriors on the device')
    r.add_argument('--error-lod-threshold', type=float, default=2.0, metavar='T',
                   help='with --diagnostics: an expressed gene whose error LOD is above T counts as flagged (default 2.0)')
    r.add_argument('--gene-report', default=None, metavar='PATH',
                   help='with --diagnostics and --sample-file: one line per gene over the samples of the cohort')
    r.add_argument('--loglik', action='store_true',
                   help='(extension) also writes <outbase>.loglik.tsv: the data log-likelihood of the sample under the '
                        'transition tables, per chromosome and in total, from what the forward pass kept on the device')
    r.add_argument('--alt-tprob-file', action='append', type=_existing, default=None, metavar='PATH',
                   help='(extension, repeatable, implies --loglik) another transition table file, e.g. the other sex or '
                        'generation: the sample is scored under every candidate on the device and reconstructed under '
                        'the one with the largest log-likelihood (-t first on ties)')
    r.add_argument('--model-report', default=None, metavar='PATH',
                   help='with --sample-file and --alt-tprob-file: one line per sample with the selected file, the margin '
                        'and the total per candidate')
    r.add_argument('--match-panel', type=_existing, default=None, metavar='FILE',
                   help='(extension, needs --grid-file) a panel of reference genotypes: tab separated lines `id<TAB>path`, each '
                        'path a dosage table on the grid as --grid-file writes it (`gbrs export` format).  The founder '
                        'dosages of every sample are compared with every entry on the device; writes <outbase>.match.tsv, '
                        'the entries by mean squared dosage difference per grid point')
    r.add_argument('--match-labels', type=_existing, default=None, metavar='FILE',
                   help='with --match-panel and --sample-file: lines `outbase<TAB>panel id`, the entry each sample should be')
    r.add_argument('--match-expected', default=None, metavar='ID',
                   help='with --match-panel and -e: the panel id the sample should be')
    r.add_argument('--match-chromosomes', default=None, metavar='LIST',
                   help='with --match-panel: comma list of the chromosomes that are compared (default: every chromosome on '
                        'the grid), e.g. the autosomes when the X chromosome of males would dominate')
    r.add_argument('--match-report', default=None, metavar='PATH',
                   help='with --match-panel and --sample-file: one line per sample with its status (match, mismatch, '
                        'unlabelled, unknown-label), the best and second entry, their distances and the margin')
    r.add_argument('--match-matrix', default=None, metavar='PATH',
                   help='with --match-panel and --sample-file: an .npz with the distances and similarities of all samples '
                        'against all entries and the sums they were made from')
    r.add_argument('--snp-file', type=_existing, default=None, metavar='FILE',
                   help='(extension) SNPs to impute from the founder haplotypes: one header line, then tab separated '
                        '`id, chr, bp, cM, pattern`, the pattern one 0/1 character per haplotype (1: the founder carries the '
                        'alternative allele); a cM of NA is filled from bp over the rows of --grid-file.  Writes '
                        '<outbase>.snp_dosage.npz: the expected number of alternative alleles at every SNP, in file order')
    r.add_argument('--snp-matrix', default=None, metavar='PATH',
                   help='with --snp-file and --sample-file: an .npz with the SNP dosages of all samples (samples x SNPs) '
                        'and the columns of the SNP file')
    r.add_argument('--scan-pheno', type=_existing, default=None, metavar='FILE',
                   help='(extension; needs --grid-file and --sample-file) genome scan: a tab separated table with the header '
                        '`id<TAB>name...`, rows keyed by outbase, one column per phenotype.  Every phenotype is regressed on '
                        'the founder dosages of the samples that ran at every grid point (Haley-Knott, on the device); writes '
                        '<PREFIX>.scan.npz and <PREFIX>.scan.peaks.tsv')
    _scan_options(r)
    r.add_argument('--scan-snps', action='store_true',
                   help='with --snp-file, --scan-pheno, --grid-file and --sample-file: every SNP of the file is tested with '
                        'one degree of freedom on the allele dosage its founder pattern implies, on the device (the cM column '
                        'in the grid file\'s position units); writes <PREFIX>.scan.snps.npz and <PREFIX>.scan.snps.peaks.tsv')
    r.add_argument('-t', '--tprob-file', required=True, type=_existing)
    r.add_argument('-x', '--avec-file', type=_existing, default=None)
    r.add_argument('-g', '--gpos-file', type=_existing, default=None)
    r.add_argument('-c', '--expr-threshold', type=float, default=1.5)
    r.add_argument('-s', '--sigma', type=float, default=0.12)
    r.add_argument('-o', '--outbase', default=None)
    r.add_argument('-v', '--verbose', action='count', default=0)
    r.add_argument('--device', type=int, default=0, help='HIP device ordinal (extension)')
    sc = sub.add_parser('scan', help='(extension) genome scan of phenotypes on exported founder dosages')
    sc.add_argument('--dosage-list', required=True, type=_existing, metavar='FILE',
                    help='lines `id<TAB>dosage table`: the samples and their tables in `gbrs export` format on the grid file')
    sc.add_argument('--grid-file', required=True, type=_existing)
    sc.add_argument('--pheno', required=True, type=_existing, metavar='FILE',
                    help='tab separated table with the header `id<TAB>name...`, rows keyed by the ids of --dosage-list')
    sc.add_argument('--covar', dest='scan_covar', type=_existing, default=None, metavar='FILE',
                    help='additive covariates: the same layout, numeric; the intercept is added')
    _scan_options(sc, covar=False)
    sc.add_argument('--snp-file', type=_existing, default=None, metavar='FILE',
                    help='SNP association after the scan: `id, chr, bp, cM, pattern` as for reconstruct --snp-file, the '
                         'haplotypes those of the dosage tables\' header, cM in the grid file\'s position units; writes '
                         '<PREFIX>.scan.snps.npz and <PREFIX>.scan.snps.peaks.tsv')
    sc.add_argument('-v', '--verbose', action='count', default=0)
    sc.add_argument('--device', type=int, default=0)
    it = sub.add_parser('interpolate', help='interpolate probability on a decently-spaced grid')
    it.add_argument('-i', '--genoprob-file', required=True, type=_existing)
    it.add_argument('-g', '--grid-file', type=_existing, default=None)
    it.add_argument('-p', '--gpos-file', type=_existing, default=None)
    it.add_argument('-o', '--output', dest='output_file', default=None)
    it.add_argument('-v', '--verbose', action='count', default=0)
    it.add_argument('--device', type=int, default=0)
    ex = sub.add_parser('export', help='export to GBRS quant format')
    ex.add_argument('-i', '--genoprob-file', required=True, type=_existing)
    ex.add_argument('-s', '--strains', action='append', required=True)
    ex.add_argument('-g', '--grid-file', type=_existing, default=None)
    ex.add_argument('-o', '--output', dest='output_file', default=None)
    ex.add_argument('-v', '--verbose', action='count', default=0)
    ex.add_argument('--device', type=int, default=0)
    cp = sub.add_parser('compress', help='compress EMASE format alignment incidence matrix')
    cp.add_argument('-i', '--emase-file', dest='emase_files', action='append', required=True)
    cp.add_argument('-o', '--output', dest='output_file', required=True)
    cp.add_argument('-c', '--comp-lib', default='zlib')
    cp.add_argument('-v', '--verbose', action='count', default=0)
    cp.add_argument('--device', type=int, default=0)
    # -h is the reference's haplotype flag here (gbrs/commands.py:38), so this subparser gets --help alone
    b2 = sub.add_parser('bam2emase', help='convert a BAM file to the EMASE format', add_help=False)
    b2.add_argument('--help', action='help', help='show this help message and exit')
    b2.add_argument('-i', '--alignment-file', required=True, type=_existing)
    b2.add_argument('-h', '--haplotype-char', dest='haplotypes', action='append', default=None,
                    help='haplotype, either one per -h option, i.e. -h A -h B -h C, or a shortcut -h A,B,C')
    b2.add_argument('-m', '--locus-ids', dest='locusid_file', required=True, type=_existing)
    b2.add_argument('-o', '--output', dest='output_file', default=None)
    b2.add_argument('-d', '--delim', default='_')
    b2.add_argument('--index-dtype', default='uint32')
    b2.add_argument('--data-dtype', default='uint8')
    b2.add_argument('-v', '--verbose', action='count', default=0)
    b2.add_argument('--device', type=int, default=0, help='HIP device ordinal (extension)')
    be = sub.add_parser('bam2ec', add_help=False,
                        help='(extension) convert BAM file(s) to equivalence classes: bam2emase + compress in one pass')
    be.add_argument('--help', action='help', help='show this help message and exit')
    be.add_argument('-i', '--alignment-file', dest='alignment_files', action='append', required=True, type=_existing_or_list,
                    help='BAM file, one per -i option (the lanes of a sample), or a shortcut -i a.bam,b.bam')
    be.add_argument('-I', '--mate-file', dest='mate_files', action='append', default=None, type=_existing_or_list,
                    help='paired-end samples aligned one end at a time: the BAM file of the second end, one per -I option '
                         'or a shortcut -I a.bam,b.bam; the k-th is the mate of the k-th -i, and only alignments that both '
                         'ends have are kept (bam2emase on each end + get-common-alignments + compress in one pass)')
    be.add_argument('-h', '--haplotype-char', dest='haplotypes', action='append', default=None,
                    help='haplotype, either one per -h option, i.e. -h A -h B -h C, or a shortcut -h A,B,C')
    be.add_argument('-m', '--locus-ids', dest='locusid_file', required=True, type=_existing)
    be.add_argument('-o', '--output', dest='output_file', required=True)
    be.add_argument('-d', '--delim', default='_')
    be.add_argument('-c', '--comp-lib', default='zlib')
    be.add_argument('--index-dtype', default='uint32')
    be.add_argument('-v', '--verbose', action='count', default=0)
    be.add_argument('--device', type=int, default=0, help='HIP device ordinal (extension)')
    # structure edits of an EMASE file (emase/commands.py:75-257, gbrs/commands.py:342-366; gbrs_amd/matops.py)
    ca = sub.add_parser('get-common-alignments', help='get the common alignments')
    ca.add_argument('-i', '--emase-file', dest='emase_files', action='append', required=True)
    ca.add_argument('-o', '--output', dest='output_file', default=None)
    ca.add_argument('-c', '--comp-lib', default='zlib')
    cb = sub.add_parser('combine', help='combine EMASE files')
    cb.add_argument('-i', '--emase-file', dest='emase_files', action='append', required=True)
    cb.add_argument('-o', '--output', dest='output_file', required=True)
    cb.add_argument('-c', '--comp-lib', default='zlib')
    pu = sub.add_parser('pull-out-unique-reads', help='keep the alignments of uniquely aligning reads')
    pu.add_argument('-i', '--alignment-file', required=True, type=_existing)
    pu.add_argument('-o', '--output', dest='output_file', required=True)
    pu.add_argument('-g', '--group-file', type=_existing, default=None)
    pu.add_argument('-s', '--shallow', action='store_true')
    pu.add_argument('-a', '--ignore-alleles', action='store_true')
    cn = sub.add_parser('count-alignments', help='count alignments')
    cn.add_argument('-i', '--alignment-file', required=True, type=_existing)
    cn.add_argument('-g', '--group-file', required=True, type=_existing)
    cn.add_argument('-o', '--outbase', default='emase')
    sr = sub.add_parser('count-shared-multireads-pairwise', help='count shared multiread pairwise alignments')
    sr.add_argument('-i', '--alignment-file', required=True, type=_existing)
    sr.add_argument('-g', '--group-file', required=True, type=_existing)
    sr.add_argument('-o', '--outbase', default='emase')
    sr.add_argument('--separate-outputs', action='store_true',
                    help='(extension) write the isoform-level matrix to <outbase>.isoforms.shared_read_counts.npz and the '
                         'gene-level matrix to <outbase>.genes.shared_read_counts.npz.  By default both levels go to the '
                         'isoforms name, as in the reference, so the gene-level matrix overwrites the isoform-level one '
                         'and the isoform-level matrix is lost')
    sn = sub.add_parser('stencil', help='apply genotype calls to multi-way alignment incidence matrix')
    sn.add_argument('-i', '--alignment-file', required=True, type=_existing)
    sn.add_argument('-G', '--genotype', dest='genotype_file', required=True, type=_existing)
    sn.add_argument('-g', '--group-file', type=_existing, default=None)
    sn.add_argument('-o', '--output', dest='output_file', default=None)
    # the two inputs of reconstruct (gbrs/commands.py:282-339; gbrs_amd/hmm_inputs.py)
    tp = sub.add_parser('get-transition-prob', help='calculate the transition probabilities between markers')
    tp.add_argument('-i', '--marker-file', required=True, type=_existing)
    tp.add_argument('-s', '--haplotypes', default='A,B')
    tp.add_argument('-m', '--mating-scheme', default='RI')
    tp.add_argument('-g', '--gamma-scale', type=float, default=0.01)
    tp.add_argument('-e', '--epsilon', type=float, default=0.000001)
    tp.add_argument('-o', '--output', dest='output_file', default='tranprob.npz')
    sp = sub.add_parser('get-alignment-spec', help='get the alignment specificity of the parental strains')
    sp.add_argument('-i', '--sample-file', required=True, type=_existing)
    sp.add_argument('-s', '--parental-strains', dest='haplotypes', action='append', required=True,
                    help='parental strain, either one per -s option, i.e. -s A -s B, or a shortcut -s A,B')
    sp.add_argument('-m', '--min-expr', type=float, default=2.0)
    for p in (ca, cb, pu, cn, sr, sn, tp, sp):
        p.add_argument('-v', '--verbose', action='count', default=0)
        p.add_argument('--device', type=int, default=0, help='HIP device ordinal (extension)')
    wk = sub.add_parser('worker', help='(extension) quantify -> reconstruct -> quantify -G of many samples in one resident process')
    wk.add_argument('--jobs', required=True, type=_existing, help='JSON list of samples, see gbrs_amd/worker.py')
    wk.add_argument('-v', '--verbose', action='count', default=0)
    wk.add_argument('--device', type=int, default=0)
    wk.add_argument('--devices', default=None,
                    help='comma-separated HIP device ordinals, or "all": one resident worker process per entry, the samples '
                         'dealt round-robin (BASELINE configs[3]: 8 samples, one per GPU; replicas only, no collective)')
    return ap


def _write_stage_times(stages, error):
    """GBRS_STAGE_TIMES=<path> (measurement aid, scripts/e2e_bench.py): the wall-clock seconds of the
    driver's stages as JSON; with GBRS_T0=<time.time() of the launcher> also the start-up time up to
    main()."""
    path = os.getenv('GBRS_STAGE_TIMES')
    if not path:
        return
    import json
    if error is not None:
        stages['error'] = f'{type(error).__name__}: {error}'
    with open(path, 'w') as fh:
        json.dump(stages, fh)


def _scan_options(parser, covar=True):
    if covar:
        parser.add_argument('--scan-covar', type=_existing, default=None, metavar='FILE',
                            help='with --scan-pheno: additive covariates, the same layout, numeric; the intercept is added')
    parser.add_argument('--scan-rankz', action='store_true',
                        help='rank-based inverse normal transform of every phenotype (average ranks on ties)')
    parser.add_argument('--scan-out', default=None, metavar='PREFIX', help='prefix of the two scan files (default: gbrs)')
    parser.add_argument('--scan-min-lod', type=float, default=None, metavar='X',
                        help='only peaks of at least this LOD go to the peaks file (default: 0.0)')
    parser.add_argument('--scan-lod-matrix', action='store_true',
                        help='keep the phenotypes x grid points LOD matrix in the .npz however large it is')
    parser.add_argument('--scan-perms', type=int, default=None, metavar='B',
                        help='permutation test on the device: B permutations of the covariate model\'s residuals '
                             '(Freedman-Lane), the same for every phenotype; the .npz gains perm_max, the levels\' genome-wide '
                             'thresholds and their inputs, the peaks file the columns pvalue and threshold_<first level>')
    parser.add_argument('--scan-perm-seed', type=int, default=None, metavar='S', help='with --scan-perms: 64-bit seed (default: 0)')
    parser.add_argument('--scan-perm-alpha', default=None, metavar='A,...',
                        help='with --scan-perms: genome-wide levels, comma separated (default: 0.05,0.1)')
    parser.add_argument('--scan-perm-chromosomes', default=None, metavar='C,...',
                        help='with --scan-perms: the maximum is taken over these chromosomes only, named as in the grid file '
                             '(default: all)')
    parser.add_argument('--scan-perm-pheno', type=_existing, default=None, metavar='FILE',
                        help='with --scan-perms: one phenotype name per line; only those are permuted (default: all)')
    parser.add_argument('--scan-mediate', action='store_true',
                        help='mediation analysis on the device: for every (phenotype, chromosome) peak of the scan every '
                             'mediator joins the covariates in turn and the peak\'s LOD is formed again; a mediator that makes '
                             'it collapse is a candidate for what lies between the locus and the phenotype.  Writes '
                             '<PREFIX>.scan.mediation.npz and <PREFIX>.scan.mediation.tsv')
    parser.add_argument('--scan-mediate-min-lod', type=float, default=None, metavar='X',
                        help='with --scan-mediate: the peaks of at least this LOD are mediated (default: 6.0, a convention '
                             'for picking peaks worth a look, not a significance threshold)')
    parser.add_argument('--scan-mediate-top', type=int, default=None, metavar='K',
                        help='with --scan-mediate: the K mediators with the lowest mediated LOD are listed per peak '
                             '(default: 5, at most 64)')
    parser.add_argument('--scan-mediator-file', type=_existing, default=None, metavar='FILE',
                        help='with --scan-mediate: the mediators, a table in the phenotypes\' format with the same ids '
                             '(default: the phenotypes themselves); --scan-rankz applies to it too')
    parser.add_argument('--scan-lod-drop', type=float, default=None, metavar='X',
                        help='LOD support intervals on the device: for every peak the nearest grid points on either side whose '
                             'LOD is at most the peak\'s minus X (the chromosome\'s ends where there is none; 1.5 is the usual '
                             'choice).  <PREFIX>.scan.npz gains support_lo, support_hi and lod_drop, the peaks file the '
                             'columns support_lo and support_hi')
    parser.add_argument('--scan-effects', action='store_true',
                        help='founder effects on the device: for every (phenotype, chromosome) peak of the scan the zero-sum '
                             'effects of all founders and their standard errors.  Writes <PREFIX>.scan.effects.npz and '
                             '<PREFIX>.scan.effects.tsv.  No mixed model, no BLUP shrinkage')
    parser.add_argument('--scan-effects-min-lod', type=float, default=None, metavar='X',
                        help='with --scan-effects: the peaks of at least this LOD get their effects (default: 6.0, as '
                             '--scan-mediate-min-lod)')
    parser.add_argument('--scan-kinship', default=None, metavar='MODE',
                        help='linear mixed model on the device: MODE loco scans every chromosome with the kinship of the '
                             'cohort\'s dosages on the other chromosomes, MODE overall with the kinship of all of them; every '
                             'phenotype\'s heritability is fitted by REML.  <PREFIX>.scan.npz gains hsq and kinship_mode, the '
                             'peaks file the column hsq.  Not with --scan-perms, --scan-snps / --snp-file, --scan-mediate, '
                             '--scan-effects or --scan-lod-drop; under the mixed model those are --scan-kinship-snps, '
                             '--scan-kinship-effects and --scan-kinship-lod-drop')
    parser.add_argument('--scan-kinship-out', action='store_true',
                        help='with --scan-kinship: write the kinship matrices and the sample ids to <PREFIX>.scan.kinship.npz')
    parser.add_argument('--scan-kinship-snps', type=_existing, default=None, metavar='FILE',
                        help='with --scan-kinship: SNP association under the mixed model on the device.  FILE has the format of '
                             '--snp-file; after the scan every SNP of it is tested with one degree of freedom under the same '
                             'kinship and the heritabilities the scan fitted.  Writes <PREFIX>.scan.snps.npz (with hsq, n_used '
                             'and kinship_mode) and <PREFIX>.scan.snps.peaks.tsv (with the column hsq)')
    parser.add_argument('--scan-kinship-effects', action='store_true',
                        help='with --scan-kinship: founder effects under the mixed model on the device.  For every (phenotype, '
                             'chromosome) peak of the scan the generalised-least-squares effects of all founders and their '
                             'standard errors, at the heritabilities the scan fitted.  Writes <PREFIX>.scan.effects.npz (with '
                             'hsq and kinship_mode) and <PREFIX>.scan.effects.tsv (with the column hsq).  No BLUP shrinkage')
    parser.add_argument('--scan-kinship-effects-min-lod', type=float, default=None, metavar='X',
                        help='with --scan-kinship-effects: the peaks of at least this LOD get their effects (default: 6.0, as '
                             '--scan-effects-min-lod)')
    parser.add_argument('--scan-kinship-lod-drop', type=float, default=None, metavar='X',
                        help='with --scan-kinship: LOD support intervals of the mixed model\'s peaks on the device, by '
                             '--scan-lod-drop\'s rule.  <PREFIX>.scan.npz gains support_lo, support_hi and lod_drop, the peaks '
                             'file the columns support_lo and support_hi after hsq')
    parser.add_argument('--scan-intcovar', default=None, metavar='NAME[,NAME...]',
                        help='with --scan-covar: interactive covariates on the device (QTL x covariate, as R/qtl2\'s intcovar).  '
                             'The named columns of the covariate table also multiply the founder dosages; after the scan a '
                             'second one gives the LOD of the full model, of the additive model and of the interaction at '
                             'every grid point.  Writes <PREFIX>.scan.int.npz and <PREFIX>.scan.int.peaks.tsv; the other '
                             'files are what they are without it.  Not with --scan-kinship')


def main(argv=None) -> int:
    import time
    t_main = time.time()
    stages = {}
    if os.getenv('GBRS_T0'):
        stages['startup'] = t_main - float(os.environ['GBRS_T0'])
    args = build_parser().parse_args(argv)
    logger = configure_logging(args.verbose)
    logger.debug(args.command)
    failure = None
    # as in the reference, failures are logged and the exit code stays 0 (commands.py:146-150)
    try:
        if args.command == 'quantify':
            if args.multiread_model not in (1, 2, 3, 4):
                raise RuntimeError('-M, --multiread-model must be one of 1, 2, 3, or 4')
            from .quantify import check_bootstrap_args
            check_bootstrap_args(args.bootstrap, args.merge_identical_rows, args.gpus)
        if args.command == 'reconstruct':
            from .hmm import ReconstructOptions      # refused here, before any file is opened
            options = ReconstructOptions.of(dict(vars(args), alt_tprob_files=args.alt_tprob_file))
            options.check(args.sample_file is not None, args.grid_file, args.tprob_file)
        if args.command == 'quantify' and args.gpus is not None:
            # N child processes, one per rank; this process opens no device
            from .sharded import launch
            launch(args, sys.argv[1:] if argv is None else list(argv), stages)
        elif args.command == 'quantify':
            from .quantify import quantify
            quantify(alignment_file=args.alignment_file, group_file=args.group_file,
                     length_file=args.length_file, genotype_file=args.genotype_file, outbase=args.outbase,
                     multiread_model=args.multiread_model, pseudocount=args.pseudocount,
                     max_iters=args.max_iters, tolerance=args.tolerance,
                     report_alignment_counts=args.report_alignment_counts,
                     report_posterior=args.report_posterior or args.posterior_values,
                     posterior_values=args.posterior_values, device=args.device,
                     merge_identical_rows=args.merge_identical_rows, stage_times=stages,
                     bootstrap=args.bootstrap, bootstrap_seed=args.bootstrap_seed,
                     keep_replicates=args.keep_replicates,
                     one_shot=True)         # the command builds one handle and exits: GBRS_EM_ONE_SHOT
        elif args.command == 'worker':
            from .worker import main as worker_main
            devices = None
            if args.devices:
                if args.devices == 'all':
                    from . import _lib
                    devices = list(range(max(1, int(_lib.load().gbrs_device_count()))))
                else:
                    devices = [int(x) for x in args.devices.split(',') if x.strip() != '']
            worker_main(args.jobs, device=args.device, devices=devices)
        elif args.command == 'compress':
            from .compress import compress
            files = [f for x in args.emase_files for f in x.split(',')]
            compress(emase_files=files, output_file=args.output_file, comp_lib=args.comp_lib, device=args.device)
        elif args.command == 'bam2emase':
            from .bam2emase import bam2emase
            haplotypes = [h for x in (args.haplotypes or []) for h in x.split(',')]
            kw = {} if args.output_file is None else {'output_file': args.output_file}     # the function's default otherwise
            bam2emase(alignment_file=args.alignment_file, haplotypes=haplotypes, locusid_file=args.locusid_file,
                      delim=args.delim, index_dtype=args.index_dtype, data_dtype=args.data_dtype, device=args.device,
                      stage_times=stages, **kw)
        elif args.command == 'bam2ec':
            from .bam2emase import bam2ec, bam2ec_paired
            files = [f for x in args.alignment_files for f in x.split(',')]
            mates = None if args.mate_files is None else [f for x in args.mate_files for f in x.split(',')]
            for f in files + (mates or []):
                if not os.path.isfile(f):
                    raise FileNotFoundError(f"File '{f}' does not exist.")
            haplotypes = [h for x in (args.haplotypes or []) for h in x.split(',')]
            if mates is not None:
                if len(mates) != len(files):
                    raise RuntimeError(f'{len(files)} -i/--alignment-file but {len(mates)} -I/--mate-file: every BAM file '
                                       'needs its second end.')
                bam2ec_paired(alignment_files=[os.path.realpath(f) for f in files],
                              mate_files=[os.path.realpath(f) for f in mates], haplotypes=haplotypes,
                              locusid_file=args.locusid_file, output_file=args.output_file, delim=args.delim,
                              comp_lib=args.comp_lib, index_dtype=args.index_dtype, device=args.device, stage_times=stages)
            else:
                bam2ec(alignment_files=[os.path.realpath(f) for f in files], haplotypes=haplotypes,
                       locusid_file=args.locusid_file, output_file=args.output_file, delim=args.delim,
                       comp_lib=args.comp_lib, index_dtype=args.index_dtype, device=args.device, stage_times=stages)
        elif args.command in ('get-common-alignments', 'combine'):
            from . import matops
            files = [f for x in args.emase_files for f in x.split(',')]
            for f in files:
                if not os.path.isfile(f):
                    raise FileNotFoundError(f"File '{f}' does not exist.")
            edit = matops.get_common_alignments if args.command == 'get-common-alignments' else matops.combine
            edit(emase_files=[os.path.realpath(f) for f in files], output_file=args.output_file,
                 comp_lib=args.comp_lib, device=args.device, stage_times=stages)
        elif args.command == 'pull-out-unique-reads':
            from .matops import pull_out_unique_reads
            pull_out_unique_reads(alignment_file=args.alignment_file, output_file=args.output_file,
                                  group_file=args.group_file, shallow=args.shallow,
                                  ignore_alleles=args.ignore_alleles, device=args.device, stage_times=stages)
        elif args.command == 'count-alignments':
            from .matops import count_alignments
            count_alignments(alignment_file=args.alignment_file, group_file=args.group_file, outbase=args.outbase,
                             device=args.device)
        elif args.command == 'count-shared-multireads-pairwise':
            from .matops import count_shared_multireads_pairwise
            count_shared_multireads_pairwise(alignment_file=args.alignment_file, group_file=args.group_file,
                                             outbase=args.outbase, device=args.device, stage_times=stages,
                                             separate_outputs=args.separate_outputs)
        elif args.command == 'stencil':
            from .matops import stencil
            stencil(alignment_file=args.alignment_file, genotype_file=args.genotype_file, group_file=args.group_file,
                    output_file=args.output_file, device=args.device, stage_times=stages)
        elif args.command == 'get-transition-prob':
            from .hmm_inputs import get_transition_prob
            get_transition_prob(marker_file=args.marker_file, haplotypes=args.haplotypes,
                                mating_scheme=args.mating_scheme, gamma_scale=args.gamma_scale, epsilon=args.epsilon,
                                output_file=args.output_file, device=args.device, stage_times=stages)
        elif args.command == 'get-alignment-spec':
            from .hmm_inputs import get_alignment_spec
            strains = [s for x in args.haplotypes for s in x.split(',')]
            get_alignment_spec(sample_file=args.sample_file, haplotypes=strains, min_expr=args.min_expr,
                               device=args.device, stage_times=stages)
        elif args.command == 'scan':
            from .scan import scan_tables
            scan_tables(dosage_list=args.dosage_list, grid_file=args.grid_file, pheno_file=args.pheno,
                        covar_file=args.scan_covar, use_rankz=args.scan_rankz, out=args.scan_out, min_lod=args.scan_min_lod,
                        lod_matrix=args.scan_lod_matrix, device=args.device, scan_perms=args.scan_perms,
                        scan_perm_seed=args.scan_perm_seed, scan_perm_alpha=args.scan_perm_alpha,
                        scan_perm_chromosomes=args.scan_perm_chromosomes, scan_perm_pheno=args.scan_perm_pheno,
                        stage_times=stages, snp_file=args.snp_file, scan_mediate=args.scan_mediate,
                        scan_mediate_min_lod=args.scan_mediate_min_lod, scan_mediate_top=args.scan_mediate_top,
                        scan_mediator_file=args.scan_mediator_file, scan_effects=args.scan_effects,
                        scan_effects_min_lod=args.scan_effects_min_lod, scan_lod_drop=args.scan_lod_drop,
                        scan_kinship=args.scan_kinship, scan_kinship_out=args.scan_kinship_out,
                        scan_kinship_snps=args.scan_kinship_snps, scan_kinship_effects=args.scan_kinship_effects,
                        scan_kinship_effects_min_lod=args.scan_kinship_effects_min_lod,
                        scan_kinship_lod_drop=args.scan_kinship_lod_drop, scan_intcovar=args.scan_intcovar)
        elif args.command == 'interpolate':
            from .postproc import interpolate
            interpolate(genoprob_file=args.genoprob_file, grid_file=args.grid_file, gpos_file=args.gpos_file,
                        output_file=args.output_file, device=args.device)
        elif args.command == 'export':
            from .postproc import export
            strains = [s for x in args.strains for s in x.split(',')]
            export(genoprob_file=args.genoprob_file, strains=strains, grid_file=args.grid_file,
                   output_file=args.output_file, device=args.device)
        elif args.sample_file is not None:
            from .hmm import read_sample_file, reconstruct_many
            samples = read_sample_file(args.sample_file)
            reconstruct_many([f for f, _ in samples], [o for _, o in samples], tprob_file=args.tprob_file,
                             avec_file=args.avec_file, gpos_file=args.gpos_file, device=args.device,
                             batch_size=args.batch_size, grid_file=args.grid_file, stage_times=stages,
                             **options.keywords(cohort=True))
        else:
            from .hmm import reconstruct
            reconstruct(expression_file=args.expression_file, tprob_file=args.tprob_file,
                        avec_file=args.avec_file, gpos_file=args.gpos_file, outbase=args.outbase,
                        device=args.device, stage_times=stages, grid_file=args.grid_file,
                        **options.keywords(cohort=False))
    except Exception as e:   # noqa: BLE001 - mirror of the reference's catch-all
        failure = e
        if logger.level == logging.DEBUG:
            logger.exception(e)
        else:
            logger.error(e)
    stages['main'] = time.time() - t_main
    _write_stage_times(stages, failure)
    return 0


def run() -> None:
    """Process entry point (`gbrs` console script, `python -m gbrs_amd`).  Everything the command leaves behind is
    on disk when main() returns, so the process ends with os._exit: the interpreter's and the HIP runtime's
    orderly teardown (module finalisers, unloading the code objects, releasing gigabytes of host arrays page by
    page) is ~0.1 s nobody waits for.  GBRS_ORDERLY_EXIT=1 keeps the ordinary exit."""
    code = main()
    if os.getenv('GBRS_ORDERLY_EXIT'):
        sys.exit(code)
    logging.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(code)


if __name__ == '__main__':
    run()
