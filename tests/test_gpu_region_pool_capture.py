"""The whole dense chain -- class_scores -> label_map -> label_regions -> Regions.embed -- captured into one graph and
replayed on new inputs: the replay must give the eager answer bit for bit, the weights table zeroed again by the call's
own launch.  Runs on the process's default queues and changes no runtime setting."""

from __future__ import annotations

import pytest
import torch

from imagescry_amd import RegionVectors, Regions, segmentation

pytestmark = pytest.mark.gpu

SIZE, ROWS = (60, 90), 32


def chain(maps: torch.Tensor, vectors: torch.Tensor) -> tuple[Regions, RegionVectors]:
    labels = segmentation.segment(maps, vectors, SIZE, min_score=-0.05)
    regions = labels.regions(min_area=5, max_regions=ROWS)
    return regions, regions.embed(maps, return_weights=True)


def fields(regions: Regions, objs: RegionVectors) -> dict[str, torch.Tensor]:
    out = {"ids": regions.ids, "num": regions.num, "label": regions.label, "area": regions.area, "mass": objs.mass,
           "weights": objs.weights, "vectors": objs.vectors.view(torch.int32)}  # bits, so that a NaN would equal itself
    return {k: v.clone() for k, v in out.items()}


def test_captured_chain_replays_on_new_inputs(device) -> None:
    g = torch.Generator().manual_seed(31)
    inputs = [(torch.randn((2, 24, 4, 6), generator=g), torch.randn((3, 24), generator=g)) for _ in range(3)]
    maps, vectors = (t.to(device).clone() for t in inputs[0])
    eager = []
    for m, v in inputs:
        eager.append(fields(*chain(m.to(device), v.to(device))))
    torch.cuda.synchronize()
    assert not torch.equal(eager[0]["ids"], eager[1]["ids"]) and int(eager[1]["num"].min()) > 1

    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        chain(maps, vectors)  # warm-up
    torch.cuda.current_stream(device).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        regions, objs = chain(maps, vectors)
    for i in (1, 2, 0, 1):
        maps.copy_(inputs[i][0])  # the inputs overwritten in place
        vectors.copy_(inputs[i][1])
        objs.weights.fill_(-3)  # garbage where the graph has to start from zero
        objs.vectors.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        got = fields(regions, objs)
        for k, want in eager[i].items():
            assert torch.equal(got[k], want), f"{k} of the replay on inputs {i} differs from the eager run"
    assert objs.label is regions.label and objs.num is regions.num
