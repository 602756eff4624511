"""CPU tier of recorded trajectories (`sample_chain`): the frame table `paths.chain_frames` against the reference's loop
(en_diffusion.py:669-710: after the step arriving at s it writes chain[(s * keep_frames) // T], later writes overwrite earlier ones),
its argument errors, and the host-side refusals of the recording entry points (raised before a GPU is touched)."""
import pytest
import torch

from hierdiff_amd import paths

T_MAX = 40


def reference_table(T, keep):
    """frame_of of the identity path from literally running the reference's loop: the last writer of every frame."""
    last = {}
    for s in reversed(range(T)):
        last[(s * keep) // T] = s
    table = [-1] * T
    for f, s in last.items():
        table[T - 1 - s] = f                      # the step arriving at s is transition k = T - 1 - s
    return table, last


def test_identity_path_is_the_reference_loop():
    for T in range(1, T_MAX + 1):
        for keep in range(1, T + 1):
            table, last = reference_table(T, keep)
            cf = paths.chain_frames(T, keep)
            assert cf.frame_of == table, (T, keep)
            assert cf.frame_t == [last[f] for f in range(keep)], (T, keep)


def test_every_frame_is_claimed_exactly_once():
    for K in range(1, T_MAX + 1):
        for keep in range(1, K + 1):
            fo = paths.chain_frames(K, keep).frame_of
            assert len(fo) == K
            assert sorted(f for f in fo if f >= 0) == list(range(keep)), (K, keep)
            assert fo[K - 1] == 0                 # the last transition arrives at position 0: frame 0 (the decode overwrites it)
            # frames fall along the chain: a later transition never writes a later frame
            kept = [f for f in fo if f >= 0]
            assert kept == sorted(kept, reverse=True)


@pytest.mark.parametrize("T,K,spacing", [(40, 7, "uniform"), (40, 13, "quadratic"), (1000, 100, "uniform"), (20, 20, "uniform")])
def test_reported_timestep_is_the_arrival_step_of_the_path(T, K, spacing):
    path = paths.build_path(T, K, spacing)
    for keep in (1, 2, K // 2 + 1, K):
        cf = paths.chain_frames(K, keep, path)
        for k, f in enumerate(cf.frame_of):
            if f >= 0:
                assert cf.frame_t[f] == path[k + 1]
                assert f == ((K - 1 - k) * keep) // K
        assert cf.frame_t[0] == 0
    part = paths.partial_path(T, T // 2, min(K, T // 2))
    cf = paths.chain_frames(len(part) - 1, 3 if len(part) > 3 else 1, part)
    assert all(cf.frame_t[f] == part[k + 1] for k, f in enumerate(cf.frame_of) if f >= 0)


@pytest.mark.parametrize("K,keep", [(6, 7), (6, 0), (6, -1), (1, 2), (20, 21)])
def test_keep_outside_1_to_K_raises(K, keep):
    with pytest.raises(ValueError, match="keep_frames"):
        paths.chain_frames(K, keep)


def test_bad_arguments_raise():
    for bad in (2.0, True, "3", None):
        with pytest.raises(ValueError):
            paths.chain_frames(6, bad)
    with pytest.raises(ValueError):
        paths.chain_frames(0, 1)
    with pytest.raises(ValueError, match="path must hold"):
        paths.chain_frames(6, 3, [6, 3, 0])


def small_model(T=20):
    from hierdiff_amd import EnVariationalDiffusion, default_config
    return EnVariationalDiffusion(default_config(hidden_nf=32, n_layers=1, timesteps=T))


def test_host_side_refusals_come_before_the_gpu():
    """Every refusal of a recording call is host arithmetic: it is raised on a CPU tensor, before the 'no CPU fallback' error."""
    from hierdiff_amd import DiffusionQM9
    m = small_model()
    nm = torch.ones(2, 3, 1, dtype=torch.bool)
    for keep in (0, 21, -3):
        with pytest.raises(ValueError, match="keep_frames"):
            m.sample_from_masks(nm, None, None, keep_frames=keep)
    with pytest.raises(ValueError, match="keep_frames"):
        m.sample_from_masks(nm, None, None, steps=6, keep_frames=7)
    with pytest.raises(ValueError, match="keep_frames"):
        m.sample_from_masks(nm, None, None, keep_frames=2.5)
    with pytest.raises(ValueError, match="record"):
        m.sample_from_masks(nm, None, None, record="x0")
    with pytest.raises(ValueError, match="record"):
        m.sample_from_masks(nm, None, None, keep_frames=4, record="eps")
    with pytest.raises(ValueError, match="record"):
        m.sample_from_latent(torch.zeros(2, 3, 11), nm, record="x0")
    with pytest.raises(ValueError, match="keep_frames"):
        m.sample_from_latent(torch.zeros(2, 3, 11), nm, t_start=12, keep_frames=13)
    with pytest.raises(ValueError, match="record"):
        m.sample_inpaint(nm, nm, torch.zeros(2, 3, 3), torch.zeros(2, 3, 8), record="x0")
    with pytest.raises(ValueError, match="keep_frames"):
        m.sample_inpaint(nm, nm, torch.zeros(2, 3, 3), torch.zeros(2, 3, 8), steps=5, keep_frames=6)
    with pytest.raises(ValueError, match="keep_frames"):
        DiffusionQM9.sample(m, 2, "cpu", steps=6, keep_frames=7)
    with pytest.raises(ValueError, match="record"):
        DiffusionQM9.sample(m, 2, "cpu", record="x0")
    with pytest.raises(NotImplementedError, match="pocket"):
        m.sample_from_masks(nm, None, None, keep_frames=4, pocket=(None,) * 4)
    m.noise_mode = "torch"
    with pytest.raises(NotImplementedError, match="noise_mode"):
        m.sample_from_masks(nm, None, None, keep_frames=4)
    with pytest.raises(NotImplementedError, match="noise_mode"):
        m.sample_chain(2, 3, nm, None, None, keep_frames=4)
    m.noise_mode = "philox"
    m.dynamics.mode = "gnn_dynamics"
    try:
        with pytest.raises(NotImplementedError, match="gnn_dynamics"):
            m.sample_from_masks(nm, None, None, keep_frames=4)
    finally:
        m.dynamics.mode = "egnn_dynamics"


def test_chain_timesteps_of_the_entry_points():
    m = small_model()
    assert m._chain_times(20).tolist() == list(range(20))
    assert m._chain_times(4, steps=6).tolist() == paths.chain_frames(6, 4, paths.uniform_path(20, 6)).frame_t
    assert m._chain_times(3, t_start=12, steps=6).tolist() == paths.chain_frames(6, 3, paths.uniform_path(12, 6)).frame_t


def test_sampler_cli_arguments():
    from hierdiff_amd import sampler
    a = sampler.parse_args(["--chain", "5", "--record", "x0", "--steps", "10"])
    assert a.chain == 5 and a.record == "x0"
    assert sampler.parse_args([]).chain is None
    for bad in (["--record", "z"], ["--chain", "0"], ["--chain", "3", "--score", "x.pkl"]):
        with pytest.raises(SystemExit):
            sampler.parse_args(bad)
