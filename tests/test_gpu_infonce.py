"""The in-batch InfoNCE kernel (avid_infonce), ops.infonce, criterions.InfoNCE and TrainStep under it, on the GPU: against
the float64 restatement within the bounds of tests/_infonce_ref.py (accepted on the CPU by tests/test_infonce_host.py), and
bit for bit where the contract says so — block decompositions, repeated runs, CU budgets, guarded buffers, the launch
programs against the per-layer path, a captured graph against eager steps."""
import numpy as np
import pytest
import torch

import _infonce_ref as R

pytestmark = pytest.mark.gpu

INV_T = 1.0 / 0.07
_CACHE = {}


def _inputs(regime, G, D, inv_T, seed=3):
    """(v, a) float32 numpy of a case: made once, shared among the tests, never written to."""
    key = (regime, G, D, inv_T, seed)
    if key not in _CACHE:
        _CACHE[key] = (R.make_unrelated if regime == "unrelated" else R.make_trained)(G, D, seed, inv_T)
    return _CACHE[key]


def _run(dev, v, a, inv_T, w=(0.5, 0.5), gs=1.0, row0=0, b=None, ws=None, place=None):
    from avid_hip import ops
    vt, at = torch.from_numpy(v).to(dev).requires_grad_(True), torch.from_numpy(a).to(dev).requires_grad_(True)
    if place is not None:
        vt, at = place(vt), place(at)
    loss, losses, hits, grads = ops.infonce(vt, at, row0=row0, b=b, inv_T=inv_T, weights=w, grad_scale=gs, ws=ws)
    torch.cuda.synchronize()
    assert loss.requires_grad and torch.equal(loss.detach().view(torch.int32), losses[0].view(torch.int32))
    return {"loss": float(losses[0]), "v2a": float(losses[1]), "a2v": float(losses[2]), "hits": tuple(int(h) for h in hits),
            "dv": grads[0].cpu().numpy(), "da": grads[1].cpu().numpy()}


def _same(x, y):
    """Two results of ``_run`` have the same bits."""
    return (all(x[k] == y[k] for k in ("loss", "v2a", "a2v", "hits"))
            and all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in ("dv", "da")))


def _check(got, v, a, inv_T, w=(0.5, 0.5), gs=1.0, row0=0, b=None):
    r = R.ref64(v, a, inv_T, w, gs, row0, b)
    bd = R.bounds(r, v, a, inv_T, w, gs, row0, b)
    ex = R.excess(got, r, bd)
    print(f"G={v.shape[0]} D={v.shape[1]} 1/T={inv_T:.4g} w={w}: loss {got['loss']:.8g} (float64 {r['loss']:.8g}), "
          f"worst error / bound {ex:.3g}, hits {got['hits']} (float64 {r['hits']})")
    assert ex <= 1.0
    assert got["hits"] == r["hits"]
    return r


# G: 1, 2, 3, around one tile (31 .. 33, 64, 65), around two (127, 129), several tiles (200) and more than one workgroup
# per direction with a partial last tile (1030); D: one staged chunk (32), the flagship width (128), four column slabs (512).
# (the wider embeddings go with the smaller batches: the makers insist on a top-two gap of ten score bounds in every row,
# and that gap closes with G while the bound opens with D)
SHAPES = [(1, 32), (2, 128), (3, 512), (31, 32), (32, 128), (33, 512), (64, 128), (65, 512), (127, 128), (129, 32), (200, 128),
          (1030, 32)]


@pytest.mark.parametrize("regime", ["unrelated", "trained"])
@pytest.mark.parametrize("G,D,tau", [(G, D, (0.07, 0.2)[i % 2]) for i, (G, D) in enumerate(SHAPES)] + [(64, 128, 0.2), (65, 512, 0.07)])
def test_kernel_against_float64(gpu_device, regime, G, D, tau):
    v, a = _inputs(regime, G, D, 1.0 / tau)
    got = _run(gpu_device, v, a, 1.0 / tau)
    _check(got, v, a, 1.0 / tau)
    if G == 1:
        assert got["loss"] == 0.0 and got["v2a"] == 0.0 and got["a2v"] == 0.0 and got["hits"] == (1, 1)
        assert not got["dv"].any() and not got["da"].any()


@pytest.mark.parametrize("case", [R.extreme_small_tau, R.extreme_identical_pairs])
def test_extreme_temperatures(gpu_device, case):
    """tau = 0.005 on unrelated rows (a fixed shift by 1 / tau gives log 0) and tau = 0.01 on identical pairs (no shift
    overflows exp): finite and inside the bounds with the row's running maximum."""
    v, a, inv_T = case()
    got = _run(gpu_device, v, a, inv_T)
    assert np.isfinite(got["loss"]) and np.isfinite(got["dv"]).all() and np.isfinite(got["da"]).all()
    _check(got, v, a, inv_T)


@pytest.mark.parametrize("regime", ["unrelated", "trained"])
@pytest.mark.parametrize("w", [(1.0, 0.0), (0.0, 1.0), (0.3, 0.7)])
def test_direction_weights(gpu_device, regime, w):
    v, a = _inputs(regime, 130, 64, INV_T)
    _check(_run(gpu_device, v, a, INV_T, w, gs=2.0), v, a, INV_T, w, gs=2.0)


def test_block_decomposition_is_bit_identical(gpu_device):
    """G = 201: blocks of 67 at 0, 67, 134, (row0, b) = (72, 56) and (200, 1) — the rows of the one b = G call, the same loss."""
    G, w, gs = 201, (0.3, 0.7), 3.0
    v, a = _inputs("trained", G, 64, INV_T)
    full = _run(gpu_device, v, a, INV_T, w, gs)
    _check(full, v, a, INV_T, w, gs)
    for row0, b in ((0, 67), (67, 67), (134, 67), (72, 56), (200, 1)):
        part = _run(gpu_device, v, a, INV_T, w, gs, row0, b)
        assert part["dv"].shape == (b, 64)
        assert np.array_equal(part["dv"].view(np.uint32), full["dv"][row0:row0 + b].view(np.uint32)), (row0, b)
        assert np.array_equal(part["da"].view(np.uint32), full["da"][row0:row0 + b].view(np.uint32)), (row0, b)
        assert (part["loss"], part["v2a"], part["a2v"], part["hits"]) == (full["loss"], full["v2a"], full["a2v"], full["hits"])


def test_duplicated_keys_tie_to_the_lowest_index(gpu_device):
    """Bit-identical key rows give bit-identical scores wherever they sit (same tile: 10 / 40, another tile: 5 / 68, and
    20 / 50 among the video rows): a row whose maximum is reached twice is a hit iff its own index is the lower one."""
    G, D = 70, 32
    v, a = (x.copy() for x in _inputs("unrelated", G, D, INV_T))
    a[68], a[40], v[50] = a[5], a[10], v[20]
    v[5] = v[68] = a[5]                  # rows 5 and 68 peak at keys 5 and 68 alike: 5 is a hit, 68 is not
    v[10] = v[40] = a[10]
    a[20] = a[50] = v[20]                # columns 20 and 50 peak at rows 20 and 50 alike
    S = (v.astype(np.float64)[:, None, :] * a.astype(np.float64)[None, :, :]).sum(-1) * INV_T     # one order for every pair
    for M in (S, S.T):                   # apart from the planted ties every row's maximum stands clear of the rest
        for row in M:
            u = np.unique(row)
            assert u[-1] - u[-2] > 10 * R.score_bound(D, INV_T)
    ar = np.arange(G)
    want = (int((S.argmax(1) == ar).sum()), int((S.argmax(0) == ar).sum()))
    assert S.argmax(1)[68] == 5 and S.argmax(1)[40] == 10 and S.argmax(0)[50] == 20 and S[5, 5] == S[5, 68]
    got = _run(gpu_device, v, a, INV_T)
    assert got["hits"] == want
    r = R.ref64(v, a, INV_T)
    assert R.excess(got, r, R.bounds(r, v, a, INV_T)) <= 1.0


def test_same_bits_on_every_run_and_cu_budget(gpu_device):
    from avid_hip import ops
    v, a = _inputs("trained", 201, 64, INV_T)
    first = _run(gpu_device, v, a, INV_T, (0.3, 0.7), 1.0, 72, 56)
    assert _same(first, _run(gpu_device, v, a, INV_T, (0.3, 0.7), 1.0, 72, 56))
    full = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        for reserve in (8, 24):
            assert ops.set_cu_budget(full - reserve) == full - reserve
            assert _same(first, _run(gpu_device, v, a, INV_T, (0.3, 0.7), 1.0, 72, 56)), reserve
    finally:
        ops.set_cu_budget(0)


def test_guarded_buffers_and_exact_workspace(gpu_device):
    """Both fills, a workspace of exactly avid_infonce_workspace_bytes: no guard byte changes, the same bits as the plain run."""
    from avid_hip import lib
    from _guards import FILLS, guarded
    G = 201
    v, a = _inputs("trained", G, 64, INV_T)
    plain = _run(gpu_device, v, a, INV_T, (0.3, 0.7), 1.0, 72, 56)
    need = int(lib.raw("avid_infonce_workspace_bytes")(G))
    for fill in FILLS:
        with guarded(fill) as g:
            got = _run(gpu_device, v, a, INV_T, (0.3, 0.7), 1.0, 72, 56, place=g.place)
            g.check()
            assert [n for n, _, _ in g.workspaces] == [need] and need in g.size_values
        assert _same(plain, got), hex(fill)


def test_criterion_end_to_end(gpu_device):
    """criterions.InfoNCE on unnormalised embeddings: loss, log and .grad against the float64 chain (normalize, scores, two
    cross-entropies, autograd).  The bound is the kernel's, with the error of the float32 normalisation (4 u per operand of
    a product: D + 8 in place of D in the score bound, 4 u |W| |a| in the gradient) carried through the normalisation's
    backward g = (d - x^ (x^ . d)) / |x| — linear in d, so a bound E on d gives (E + |x^| (|x^| . E)) / |x| — plus that
    backward's own D + 6 roundings on the magnitudes."""
    import criterions
    G, D, tau, coeff = 37, 128, 0.1, (1.0, 3.0)
    rng = np.random.RandomState(5)
    e1 = (rng.randn(G, D) * 1.7).astype(np.float32)
    e2 = (0.8 * e1 + 0.6 * rng.randn(G, D) * 1.7).astype(np.float32)
    crit = criterions.InfoNCE(D, device=0, temperature=tau, v2a_coeff=coeff[0], a2v_coeff=coeff[1], num_data=1000)
    t1, t2 = (torch.from_numpy(e).to(gpu_device).requires_grad_(True) for e in (e1, e2))
    loss, log = crit(t1, t2, torch.arange(G, device=gpu_device))
    loss.backward()
    x1, x2 = (torch.tensor(e, dtype=torch.float64, requires_grad=True) for e in (e1, e2))
    n1, n2 = torch.nn.functional.normalize(x1, dim=1), torch.nn.functional.normalize(x2, dim=1)
    S = n1 @ n2.t() / tau
    tgt = torch.arange(G)
    lv, la = torch.nn.functional.cross_entropy(S, tgt), torch.nn.functional.cross_entropy(S.t(), tgt)
    ref = 0.25 * lv + 0.75 * la
    ref.backward()
    v, a = n1.detach().numpy(), n2.detach().numpy()
    w = (0.25, 0.75)
    r = R.ref64(v, a, 1.0 / tau, w)
    wide = np.zeros((G, 8))                      # eight columns of zeros: D + 8 in the bounds, nothing else changes
    bd = R.bounds(r, np.concatenate([v, wide], 1), np.concatenate([a, wide], 1), 1.0 / tau, w)
    assert abs(float(loss.detach()) - float(ref.detach())) <= bd["loss"] and abs(float(log["Loss/v2a"]) - float(lv.detach())) <= bd["v2a"]
    assert abs(float(log["Loss/a2v"]) - float(la.detach())) <= bd["a2v"]
    assert float(log["Acc/v2a"]) == 100.0 * r["hits"][0] / G and float(log["Acc/a2v"]) == 100.0 * r["hits"][1] / G
    assert sorted(log) == ["Acc/a2v", "Acc/v2a", "Loss/a2v", "Loss/v2a"]
    absW = np.abs(r["W"])
    for got, x, xh, d, E, Wk, keys in ((t1.grad, e1, v, r["dv"], bd["dv"][:, :D], absW, a), (t2.grad, e2, a, r["da"], bd["da"][:, :D], absW.T, v)):
        nrm = np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
        E = E + 4 * R.U * (Wk @ np.abs(keys))
        mag = np.abs(d) + np.abs(xh) * (np.abs(xh) * np.abs(d)).sum(1, keepdims=True)
        Eg = (E + np.abs(xh) * (np.abs(xh) * E).sum(1, keepdims=True)) / nrm + (D + 6) * R.U * R.SLACK * mag / nrm
        want = (x1.grad if x is e1 else x2.grad).numpy()
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print("criterion grad: worst error / bound", float((err / Eg).max()))
        assert (err <= Eg).all()


# ------------------------------------------------------------------------------------------------ TrainStep under InfoNCE
def _engine(dev, **kw):
    import criterions
    import test_gpu_two_ranks as T2
    from avid_hip.parallel import TrainStep
    m = T2._model(dev)
    crit = criterions.InfoNCE(128, device=0, temperature=0.07)
    return m, crit, TrainStep(m, crit, bucket_bytes=4 << 20, **kw)


def _clips(dev):
    import test_gpu_two_ranks as T2
    video, audio = T2._inputs()
    return video.to(dev), audio.to(dev), torch.arange(video.shape[0], device=dev)


def _state(eng):
    return [t.clone() for t in (eng.flat.flat, eng.m, eng.v)]


def _bits(x, y):
    return x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.fixture(scope="module")
def program_steps(gpu_device):
    """Two steps through the launch programs: (losses, state after each step)."""
    video, audio, ids = _clips(gpu_device)
    m, crit, eng = _engine(gpu_device)
    losses, states = [], []
    for _ in range(2):
        losses.append(float(eng.step(video, audio, ids)))
        states.append(_state(eng))
    assert eng._step_plan is not None, "the step did not run through the launch programs"
    assert all(np.isfinite(l) for l in losses) and not _bits(states[0][0], states[1][0])
    return losses, states


def test_trainstep_programs_equal_the_per_layer_path(gpu_device, program_steps, per_layer_path):
    video, audio, ids = _clips(gpu_device)
    m, crit, eng = _engine(gpu_device)
    for i in range(2):
        assert float(eng.step(video, audio, ids)) == program_steps[0][i]
        assert eng._step_plan is None
        assert all(_bits(x, y) for x, y in zip(_state(eng), program_steps[1][i])), i


def test_trainstep_capture_replay_equals_eager(gpu_device, program_steps):
    video, audio, ids = _clips(gpu_device)
    m, crit, eng = _engine(gpu_device)
    m2, crit2, twin = _engine(gpu_device)
    for i in range(2):
        eng.step(video, audio, ids)
        twin.step(video, audio, ids)
    assert all(_bits(x, y) for x, y in zip(_state(eng), program_steps[1][1]))
    eng.capture(video, audio, ids)
    torch.cuda.synchronize()
    assert all(_bits(x, y) for x, y in zip(_state(eng), program_steps[1][1]))          # the capture ran nothing
    for i in range(2):
        got = eng.replay(index=ids)
        want = twin.step(video, audio, ids)
        torch.cuda.synchronize()
        assert float(got) == float(want)
        assert all(_bits(x, y) for x, y in zip(_state(eng), _state(twin))), i
    assert not _bits(eng.flat.flat, program_steps[1][1][0])


def test_trainstep_skips_a_non_finite_step(gpu_device, program_steps):
    """skip_nonfinite, a NaN planted in the clip of the second step: parameters and optimizer state stay untouched (there is
    no bank to put back); the first step is the unguarded one bit for bit."""
    video, audio, ids = _clips(gpu_device)
    m, crit, eng = _engine(gpu_device, skip_nonfinite=True)
    eng.step(video, audio, ids)
    assert int(eng.guard.skipped) == 0 and all(_bits(x, y) for x, y in zip(_state(eng), program_steps[1][0]))
    before = _state(eng)
    bad = video.clone()
    bad[1, 1, 3, 17, 29] = float("nan")
    eng.step(bad, audio, ids)
    assert int(eng.guard.skipped) == 1 and int(eng.guard.skipped_total) == 1
    assert all(_bits(x, y) for x, y in zip(_state(eng), before))
    eng.step(video, audio, ids)
    assert int(eng.guard.skipped) == 0 and all(_bits(x, y) for x, y in zip(_state(eng), program_steps[1][1]))


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "lars", "lamb"])
def test_trainstep_optimizers_ema_and_param_rules(gpu_device, optimizer):
    """Every optimizer of the step engine with per-tensor rules and the weight average, two steps through the launch programs:
    finite losses, parameters and average move, the average trails the parameters, nothing is skipped."""
    from avid_hip import parallel
    import criterions
    import test_gpu_two_ranks as T2
    video, audio, ids = _clips(gpu_device)
    m = T2._model(gpu_device)
    kw = dict(momentum=0.9) if optimizer in ("sgd", "lars") else {}
    eng = parallel.TrainStep(m, criterions.InfoNCE(128, device=0), lr=1e-3, optimizer=optimizer, ema_decay=0.9,
                             param_rules=parallel.rules_no_decay_1d(m), max_grad_norm=1e3, skip_nonfinite=True, **kw)
    start = eng.flat.flat.clone()
    losses = [float(eng.step(video, audio, ids)) for _ in range(2)]
    assert eng._step_plan is not None and all(np.isfinite(l) for l in losses)
    assert int(eng.guard.skipped_total) == 0 and int(eng.ema_updates) == 2
    assert bool(torch.isfinite(eng.flat.flat).all()) and bool(torch.isfinite(eng.ema).all())
    assert not _bits(eng.flat.flat, start) and not _bits(eng.ema, start) and not _bits(eng.ema, eng.flat.flat)


def test_device_arguments_are_refused_before_launch(gpu_device, kernel_log):
    from avid_hip import AvidHipError, ops
    import criterions
    x = torch.zeros((8, 64), device=gpu_device)
    with kernel_log() as log:
        for kw in (dict(row0=-1), dict(row0=5, b=4), dict(b=-1), dict(inv_T=0.0), dict(inv_T=float("inf")), dict(weights=(-1.0, 1.0)),
                   dict(weights=(0.5,)), dict(grad_scale=float("nan")), dict(ws=torch.empty(255, dtype=torch.uint8, device=gpu_device)),
                   dict(ws=torch.empty(256, dtype=torch.uint8))):
            with pytest.raises(AvidHipError):
                ops.infonce(x, x, **kw)
        for shape in ((8, 48), (8, 544), (0, 64)):
            with pytest.raises(AvidHipError):
                ops.infonce(torch.zeros(shape, device=gpu_device), torch.zeros(shape, device=gpu_device))
        with pytest.raises(AvidHipError):
            criterions.InfoNCE(128)(x, x, None)                       # built for another width
        with pytest.raises(AvidHipError):
            criterions.InfoNCE(64)(x, x[:4], None)
    assert log.launches("infonce") == 0
