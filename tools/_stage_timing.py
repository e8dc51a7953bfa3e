"""How the ``tools/*_time.py`` of the stages behind the mel layers take their figures: device events over alternated trains of calls, and graphs
of ``PER_GRAPH`` calls on static buffers (what the device spends, without the host's share of an eager call).  One copy for the six tools."""
import torch

ROUNDS = 5
PER_GRAPH = 20


def _train(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def _alternated(variants):
    """{name: (fn, calls per train)} -> {name: [us per call of each train]}, the variants taking turns"""
    for fn, _ in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, (fn, calls) in variants.items():
            times[k].append(_train(fn, calls))
    return times


def _graphed(fn, per_graph=PER_GRAPH):
    """``per_graph`` calls of fn captured into one graph: its replay is the device's time for them, without the host's"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(per_graph):
            fn()
    return graph.replay
