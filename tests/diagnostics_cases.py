"""Problems of the diagnostics tests (tests/test_diagnostics_cpu.py, tests/test_diagnostics_gpu.py): plain numpy."""
import dataclasses
import functools

import numpy as np

import grid_cases

PLANT_CHROM, PLANT_GENE, SILENT_GENE = "4", 30, 10
PLANT_TABLE = [(3, "benign"), (3, "do"), (8, "benign"), (8, "do")]


def unit(v):
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def planted(H, style):
    """grid_cases.problem(H, style) with chromosome "4" (65 genes) rewritten: every gene expresses founders 0 and 1 as its
    own specificity rows show them, 20 (unit(avec[0]) + unit(avec[1])); gene 30 shows founder 2 alone, 40 unit(avec[2]),
    which its neighbours contradict; gene 10 has 0.01 everywhere and is unexpressed.  A gene without a specificity block
    takes the naive one, as the emission does."""
    p = grid_cases.problem(H, style)
    naive = np.eye(H) + (np.ones((H, H)) - np.eye(H)) * 0.0001
    expr = dict(p.expr)
    for k, g in enumerate(p.gene_ids[PLANT_CHROM]):
        av = p.avecs.get(g, naive)
        if k == PLANT_GENE:
            expr[g] = 40.0 * unit(av[2])
        elif k == SILENT_GENE:
            expr[g] = np.full(H, 0.01)
        else:
            expr[g] = 20.0 * (unit(av[0]) + unit(av[1]))
    return dataclasses.replace(p, expr=expr)


def gap_of_the_planted_gene(errlod, expressed):
    """(the planted gene's error LOD minus the largest other one, whether the silent gene is expressed)."""
    errlod = np.asarray(errlod)
    others = np.delete(errlod, PLANT_GENE)
    return float(errlod[PLANT_GENE] - others.max()), bool(expressed[SILENT_GENE])
