"""-m gpu: _lib.call, the one path from a wrapper to an entry point - what it marshals and what it refuses - and one wrapper
per pair of branches that differ only in the entry point's name, down both branches, against the C oracle.  Tiny boards
(N = 2 and N = 5, B = 3): the kernels are pinned elsewhere, this is about the arguments."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

B = 3
SIZES = (2, 5)


@pytest.fixture(scope='module')
def starts():
    """{N: (uint8 [B, 6, N, N] positions a few plies in, uint64 [B] generators)}, on the host; never modified."""
    from gymgo_amd import gogame
    from oracle import c_oracle
    res = {}
    for N in SIZES:
        rng = gogame.rng_seed(B, 40 + N).cpu().numpy().view(np.uint64)
        states, rng, _ = c_oracle.batch_rollout(np.zeros((B, 6, N, N), np.uint8), rng, N, True)
        res[N] = (states, rng)
    return res


def _dev(starts, N):
    states, rng = starts[N]
    return torch.from_numpy(states.copy()).cuda(), torch.from_numpy(rng.view(np.int64).copy()).cuda()


def _stream():
    from gymgo_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


@pytest.mark.parametrize('N', SIZES)
def test_call_refuses_what_dev_ptr_refuses_and_launches_nothing(starts, N):
    from gymgo_amd import _lib
    from oracle import c_oracle
    st, _ = _dev(starts, N)
    black, white = (torch.full((B,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    strided = torch.full((2 * B,), -7, dtype=torch.int32, device='cuda')
    for args, name in (((st.to(torch.int32), black, white), 'states'),          # the wrong dtype
                       ((st, black.to(torch.int64), white), 'black'),
                       ((st, black, strided[::2]), 'white'),                       # not contiguous
                       ((st.cpu(), black, white), 'states'),                       # on the host
                       ((st, black, white.cpu().numpy()), 'white')):               # not a tensor
        with pytest.raises(_lib.GymGoNativeError, match=r'^%s must be ' % name):
            _lib.call('gg_batch_areas', *args, B, N, _stream())
    torch.cuda.synchronize()
    assert bool((black == -7).all()) and bool((white == -7).all()) and bool((strided == -7).all())
    with pytest.raises(TypeError, match='gg_batch_areas'):
        _lib.call('gg_batch_areas', st, black, white, B, N)
    # tensors, and the same buffers as pointers the caller has prepared
    _lib.call('gg_batch_areas', st, black, white, B, N, _stream())
    b2, w2 = (torch.full((B,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
    _lib.call('gg_batch_areas', st.data_ptr(), *_lib.ptrs('gg_batch_areas', black=b2, white=w2), B, N, _stream())
    want = c_oracle.batch_areas(starts[N][0])
    for got in ((black, white), (b2, w2)):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    with pytest.raises(_lib.GymGoNativeError, match=r'^black must be '):
        _lib.ptrs('gg_batch_areas', black=b2.to(torch.int64))


@pytest.mark.parametrize('N', SIZES)
def test_call_passes_none_as_null(starts, N):
    """last_actions and steps_done of gg_batch_rollout are nullable: None goes down as NULL."""
    from gymgo_amd import _lib
    from oracle import c_oracle
    st, rng = _dev(starts, N)
    _lib.call('gg_batch_rollout', st, rng, None, None, B, N, 3, 1, _stream())
    want, want_rng, _ = c_oracle.batch_rollout(*starts[N], 3, True)
    assert np.array_equal(st.cpu().numpy(), want) and np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng)


@pytest.mark.parametrize('N', SIZES)
def test_call_takes_every_dtype_of_a_set(starts, N):
    """todo of gg_puct_root_noise is uint8_t * and takes bool or uint8 tensors: both are accepted and do the same."""
    from gymgo_amd import _lib, gogame
    A = N * N + 1
    noise = torch.rand((B, A), dtype=torch.float32, device='cuda')
    priors = []
    for dtype in (torch.bool, torch.uint8):
        search = gogame.PuctSearch(_dev(starts, N)[0], 2)
        _, legal = search.select()
        search.backup(legal.to(torch.float32) / legal.sum(dim=1, keepdim=True).clamp(min=1), torch.zeros(B, device='cuda'))
        boards, _, prior, _, stats, nodes = search._tree
        todo = torch.ones(B, dtype=dtype, device='cuda')
        _lib.call('gg_puct_root_noise', B, N, search._C, 0.25, noise, todo, boards, prior, stats, nodes, _stream())
        live = torch.from_numpy(starts[N][0][:, 5, 0, 0] == 0).cuda()
        assert torch.equal(todo != 0, ~live)          # cleared exactly where the root was changed
        priors.append(search.result().priors.clone())
        with pytest.raises(_lib.GymGoNativeError, match=r'^todo must be '):
            _lib.call('gg_puct_root_noise', B, N, search._C, 0.25, noise, todo.to(torch.int32), boards, prior, stats, nodes, _stream())
    assert torch.equal(priors[0], priors[1])


def test_call_names_the_function_that_refused_its_arguments():
    """B = 2, N = 20: the library's own size check answers before any pointer is looked at; no kernel is launched."""
    from gymgo_amd import _lib
    with pytest.raises(_lib.GymGoNativeError, match=r'^gg_batch_next_states failed with code -1 '):
        _lib.call('gg_batch_next_states', None, None, None, None, 2, 20, 0, None)
    with pytest.raises(_lib.GymGoNativeError, match=r'^gg_batch_play_moves_packed failed with code -1 '):
        _lib.call('gg_batch_play_moves_packed', None, None, None, 2, 20, 1, None)


@pytest.mark.parametrize('N', SIZES)
def test_rollout_without_and_with_a_workspace(starts, N):
    from gymgo_amd import gogame
    from oracle import c_oracle
    want, want_rng, want_last = c_oracle.batch_rollout(*starts[N], 2 * N, True)
    for workspace in (None, gogame.next_states_workspace(B, N, 'cuda')):
        st, rng = _dev(starts, N)                     # (a new tensor: without a workspace of its own on its first call)
        la = torch.full((B,), -9, dtype=torch.int32, device='cuda')
        sd = torch.zeros(B, dtype=torch.int64, device='cuda')
        assert gogame.batch_rollout(st, rng, 2 * N, True, la, sd, workspace=workspace) is st
        assert np.array_equal(st.cpu().numpy(), want) and np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng)
        assert np.array_equal(la.cpu().numpy(), want_last) and sd.tolist() == [2 * N] * B
    with pytest.raises(ValueError):
        gogame.batch_rollout(st, rng, 1, workspace=torch.zeros((B, 5 * N), dtype=torch.int32, device='cuda'))


@pytest.mark.parametrize('N', SIZES)
def test_tracked_rollout_under_both_policies(starts, N):
    import mc_policy_expect as mp
    from gymgo_amd import gogame
    from oracle import c_oracle
    plies = 2 * N
    expect = {'uniform': c_oracle.batch_rollout(*starts[N], plies, False),
              'no_eye_fill': mp.policy_rollout(*starts[N], plies, False)[:3]}
    for policy, (want, want_rng, want_last) in expect.items():
        st, rng = _dev(starts, N)
        tracked = gogame.batch_track(st)
        la = torch.full((B,), -1, dtype=torch.int32, device='cuda')
        assert gogame.batch_rollout_tracked(tracked, rng, plies, False, la, policy=policy) is tracked
        assert np.array_equal(gogame.batch_untrack(tracked).cpu().numpy(), want), policy
        assert np.array_equal(rng.cpu().numpy().view(np.uint64), want_rng), policy
        assert np.array_equal(la.cpu().numpy(), want_last), policy


@pytest.mark.parametrize('N', SIZES)
def test_play_moves_on_bytes_and_on_packed_boards(starts, N):
    from gymgo_amd import gogame
    from oracle import c_oracle
    T = 4
    moves = np.random.default_rng(N).integers(-1, N * N + 2, size=(B, T)).astype(np.int32)
    want, played = starts[N][0].copy(), np.zeros(B, np.int32)
    for b in range(B):
        for a in moves[b]:
            s = want[b]
            if s[5, 0, 0] or not 0 <= a <= N * N or (a < N * N and s[3].reshape(-1)[a]):
                break
            want[b] = c_oracle.next_state(s, int(a))
            played[b] += 1
    st, _ = _dev(starts, N)
    packed = gogame.batch_pack(st)
    for boards in (st, packed):
        got = gogame.batch_play_moves(boards, torch.from_numpy(moves).cuda())
        assert np.array_equal(got.cpu().numpy(), played)
    assert np.array_equal(st.cpu().numpy(), want) and torch.equal(gogame.batch_unpack(packed, N), st)
