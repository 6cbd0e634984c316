"""MI355X-native evaluator back end for FeynmanDiagram.jl's static
computational graphs (package directory ``feynmandiagram.jl_amd``; import it as
``feynmandiagram_jl_amd`` through the loader module at the repository root).

Scope: the graph *evaluation* hot path only --
``Compilers.compile`` -> ``eval_graph!(root, leafVal)`` -- behind the C ABI of
include/fdg.h, plus the host-side mirror of the reference interface for it.
The restated producers of the benchmark graphs (Parquet / GV / optimize! / Taylor) live in ``producers/``: workload
generators for tests and bench.py, not product, and not exported here.
"""
from . import graph as ComputationalGraphs
from . import compilers as Compilers
from . import frontends as FrontEnds
from .graph import (FeynmanGraph, Graph, PostOrderDFS, Power, Prod, Sum, Unitary, constant_graph, eval_,
                    external_vertex, linear_combination, multi_product)
from .nodetable import NodeTable, synthetic_parquet_like, from_program
from .lowering import lower
from .compilers import GraphFunc, compile_table, mc_covariance, mc_estimate
from .vegas import DiscreteMap, MatsubaraProjection, PolarVar, Stratification, VegasMap, WeightGroups, groups_from_dof, ball, strat_for, uniform_cdf, uniform_grid, vegas_integrate, vegas_integrate_binned, vegas_integrate_stratified, ChainResult, chain_estimate, chain_integrate, chain_integrate_grouped, chain_integrate_binned, chain_integrate_polar, chain_moves_polar, ChainShift, chain_integrate_shift, chain_moves_shift, chain_estimate_observables, chain_integrate_observables, ChainObservablesResult

__all__ = ["ComputationalGraphs", "Compilers", "FrontEnds", "Graph", "FeynmanGraph", "Sum", "Prod", "Power", "Unitary",
           "constant_graph", "eval_", "external_vertex", "linear_combination", "multi_product", "PostOrderDFS",
           "NodeTable", "synthetic_parquet_like", "from_program", "lower", "GraphFunc", "compile_table", "mc_estimate", "mc_covariance",
           "VegasMap", "uniform_grid", "vegas_integrate", "DiscreteMap", "uniform_cdf", "vegas_integrate_binned", "PolarVar", "ball", "MatsubaraProjection", "WeightGroups", "groups_from_dof", "Stratification", "strat_for", "vegas_integrate_stratified", "ChainResult", "chain_estimate", "chain_integrate", "chain_integrate_grouped", "chain_integrate_binned", "chain_integrate_polar", "chain_moves_polar", "ChainShift", "chain_integrate_shift", "chain_moves_shift", "chain_estimate_observables", "chain_integrate_observables", "ChainObservablesResult"]
