"""The int8 filter levels on banks built to defeat their bound (tests/shadow_adversary.py: the families A .. F and what makes
each one tight; tests/test_shadow_adversary_host.py: the proof, in the host model, that the very banks searched here
lose a victim to a threshold that is too tight by half, to the record of the neighbouring tile or query, or to a missing
term -- faults the iid banks of tests/test_gpu_shadow.py and tests/test_gpu_shadow_levels.py cannot see).

Every case searches once on the int8 shadow and once with `shadow=False` on the same bank object:

  * scores and indices are bit-identical between the two paths, for every query of the call;
  * for the adversarial queries they are bit-identical to `search_exhaustive`, and every victim is among the indices;
  * the int8 search overflowed, redid and handed to the exhaustive pass exactly as often as the fp16 search;
  * the fp16 search of the adversarial queries ALONE redoes nothing (status[1] = status[3] = 0): the redo, an fp16 filter
    over the whole bank, would rescue a victim that an int8 level dropped -- so a dropped victim shows in the answer.
    Family F is exempt: its answer is a tie at the kp-th score, which the guard cannot prove in either path;
  * status[2] < 1: no filter score was further from the exact dot than the guard's eps.

The banks are built on the host, by the builders the host test checks, and copied to the device one at a time."""

from __future__ import annotations

import numpy as np
import pytest
import shadow_adversary as sa
import torch

pytestmark = pytest.mark.gpu


def _status(bank) -> list:
    st = bank.last_status.cpu()
    return [int(st[0]), int(st[1]), st[2:3].view(torch.float32).item(), int(st[3])]


def _same(a, b) -> None:
    assert torch.equal(a[1], b[1])
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("name", list(sa.CASES))
def test_adversarial_bank(name: str, device: torch.device) -> None:
    from imagescry_amd import EmbeddingBank

    case = sa.build_case(name)
    lay = case.layout
    assert lay.kinds == case.kinds and 2 in lay.kinds  # isc_cosine_topk_plan, not memory
    assert lay.q > 256 and len(case.adv) <= 64
    case.check_filler()  # float64 dots on the host: nothing but a query's planted rows reaches its pace-setters

    bank = EmbeddingBank(case.rows.to(device), dtype=torch.float16, normalize=False)
    queries = case.queries.to(device)
    k = lay.k
    bank.shadow = True
    got = bank.search(queries, k)
    assert bank._shadow is not None, "the plan holds no int8 level"
    status = _status(bank)
    bank.shadow = False
    ref = bank.search(queries, k)
    ref_status = _status(bank)
    adv = torch.tensor(case.adv, device=device)
    alone = bank.search(queries[adv], k)
    alone_status = _status(bank)
    exact = bank.search_exhaustive(queries[adv], k)
    bank.shadow = True
    print(f"\n{name}: status int8 {status} fp16 {ref_status} fp16, adversarial queries alone {alone_status}")

    _same(got, ref)
    _same((got[0][adv], got[1][adv]), exact)
    _same(alone, exact)
    found = got[1][adv].cpu().tolist()
    for a, qi in enumerate(case.adv):
        assert set(case.victims[qi]) <= set(found[a]), (name, qi)
    assert (status[0], status[1], status[3]) == (ref_status[0], ref_status[1], ref_status[3]), (status, ref_status)
    if case.family != "F":
        assert (alone_status[1], alone_status[3]) == (0, 0), alone_status
    for st in (status, ref_status, alone_status):
        assert 0.0 <= st[2] < 1.0, st
