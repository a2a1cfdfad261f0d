"""GoVecEnv - B independent games on ONE device (no reference counterpart: the reference has one game per GoEnv; this
is the batched form its gogame.batch_* functions imply).

One process drives one GPU; to use several GPUs run one process per GPU with `shard(rank, world)` slices of the game
range - games never interact, so there is no collective on the data path.

Three resident layouts (`layout=`):
  'tracked' (default)  int32 [B, 5N+1]: bit-packed boards that carry their liberty classes.  A step needs no per-ply
             liberty analysis (gg_batch_env_step_tracked, the multi-ply kernel run for one ply) and writes the uint8
             [B,6,N,N] observation in the same launch; `states` is that observation buffer (refreshed lazily after
             rollouts) - treat it as read-only, assign `env.states = x` to load positions.
  'bytes'    uint8 [B,6,N,N] is the resident state itself (every step re-analyses every board: gg_batch_env_step).
  'packed'   int32 [B, 3N+1] bit-packed boards without classes (gg_batch_*_packed); `states` unpacks on demand.
"""
import torch

from gymgo_amd import _lib, gogame, govars

_TRACKED_STEP = 'gg_batch_env_step_tracked'   # the entry point of the prepared step


def shard(total_games, rank, world_size):
    """Contiguous equal split of the game index range [0, total_games) -> (first_game, count)."""
    base, rem = divmod(total_games, world_size)
    first = rank * base + min(rank, rem)
    return first, base + (1 if rank < rem else 0)


class GoVecEnv:
    def __init__(self, batch_size, size, komi=0, reward_method='real', device=None, seed=20260927, first_game=0,
                 auto_reset=True, packed=False, layout=None):
        self.batch_size, self.size, self.komi = batch_size, size, komi
        self.reward_method = reward_method
        self.device = torch.device(device) if device is not None else gogame._device()
        if self.device.type == 'cuda' and self.device.index is None:
            # an INDEXED device from here on: 'cuda' means "whatever is current NOW" - resolved again at every step it would
            # name another device's stream once the caller switches devices, while the kernels follow the tensors
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.auto_reset = auto_reset
        if packed and layout not in (None, 'packed'):
            raise ValueError("packed=True is the legacy spelling of layout='packed'; it contradicts layout=%r" % (layout,))
        self.layout = layout or ('packed' if packed else 'tracked')
        if self.layout not in ('tracked', 'bytes', 'packed'):
            raise ValueError("layout must be 'tracked', 'bytes' or 'packed'")
        self.packed = self.layout == 'packed'
        if self.layout == 'packed':
            self.packed_states = torch.zeros((batch_size, gogame.packed_words(size)), dtype=torch.int32, device=self.device)
        elif self.layout == 'tracked':
            self.tracked = torch.zeros((batch_size, gogame.tracked_words(size)), dtype=torch.int32, device=self.device)
            self._obs = gogame.batch_init_state(batch_size, size, device=self.device)
            self._obs_fresh = True          # the observation buffer shows the tracked boards
        else:
            self._states = gogame.batch_init_state(batch_size, size, device=self.device)
        self.rng = gogame.rng_seed(batch_size, seed, first_game, self.device)
        self.steps_done = torch.zeros(batch_size, dtype=torch.int64, device=self.device)
        self.last_actions = torch.full((batch_size,), -1, dtype=torch.int32, device=self.device)
        # step() outputs live in fixed buffers (rewards, dones, status; the action taken goes to last_actions): no
        # allocation per step, and the step can be captured in a hipGraph.  They are overwritten by the next step.
        self._prep = None   # step(): the validated pointers of the tracked step (see there)
        self._step_out = (torch.empty(batch_size, dtype=torch.float32, device=self.device),
                          torch.empty(batch_size, dtype=torch.uint8, device=self.device),
                          torch.empty(batch_size, dtype=torch.int32, device=self.device), self.last_actions)

    @property
    def states(self):
        """uint8 [B,6,N,N] view of the games (the resident tensor itself only with layout='bytes')."""
        if self.layout == 'packed':
            return gogame.batch_unpack(self.packed_states, self.size)
        if self.layout == 'tracked':
            if not self._obs_fresh:
                gogame.batch_untrack(self.tracked, out=self._obs)
                self._obs_fresh = True
            return self._obs
        return self._states

    @states.setter
    def states(self, value):
        if self.layout == 'packed':
            self.packed_states = gogame.batch_pack(value)
        elif self.layout == 'tracked':
            self.tracked.copy_(gogame.batch_track(value.contiguous()))
            self._obs.copy_(value)
            self._obs_fresh = True
        else:
            self._states = value

    def _store(self):
        return {'packed': lambda: self.packed_states, 'tracked': lambda: self.tracked, 'bytes': lambda: self._states}[self.layout]()

    def _store_done(self):
        """bool [B]: the game-over flag of every resident game."""
        if self.layout == 'bytes':
            return self._states[:, govars.DONE_CHNL, 0, 0] != 0
        return (self._store()[:, -1] & 4) != 0

    def reset(self, mask=None):
        store = self._store()
        if mask is None:
            store.zero_()
        else:
            store[mask] = 0                  # an all-zero packed / tracked board is the empty board
        if self.layout == 'tracked':
            self._obs_fresh = False
        return self.states

    def valid_moves(self):
        return gogame.batch_valid_moves(self.states)

    def sample_actions(self):
        """Uniform over valid actions incl. pass, per game, on the device."""
        return gogame.batch_sample_actions(self.states, self.rng)

    def step(self, actions=None, check=False, probs=None):
        """One GoEnv.step per game in ONE launch -> (states, rewards, dones, status); `states` is the uint8 observation
        (layout 'tracked': written by the step itself; 'bytes': the resident tensor; 'packed': the packed tensor).
        actions=None draws a uniform-random valid action per game on the device (it is left in self.last_actions).
        probs = float32 [B, N*N+1] policy weights (need not be normalised): the move of every game is drawn from them,
        masked by the game's invalid moves, on the device (gogame.random_weighted_action, gym_go/gogame.py:385-392) - by
        the step launch itself with layout 'tracked', by one sampling launch before it otherwise; the drawn moves are
        left in self.last_actions, a game without a positive playable weight is refused (status 1).
        Finished games are reset first when auto_reset; rewards are float32, black's perspective
        (gym_go/envs/go_env.py:128-149).  The returned tensors are fixed buffers, overwritten by the next step()."""
        if actions is not None and probs is not None:
            raise ValueError('give actions OR probs, not both')
        if actions is not None:
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if probs is not None and self.layout != 'tracked':
            # (a finished game is reset by the step before the move is checked, so it is drawn for on the empty board;
            # without auto_reset it is frozen and draws NOTHING, as in the fused step of layout 'tracked': its generator
            # is put back and its move is -1 - the layouts walk the same games and the same generator streams)
            over = self._store_done()
            if self.auto_reset:
                self.reset(over)
            else:
                rng_before = self.rng.clone()
            actions = (gogame.batch_sample_weighted(self._states, probs, self.rng) if self.layout == 'bytes' else
                       gogame.batch_sample_weighted_rows(self.packed_states, self.size, probs, self.rng))
            if not self.auto_reset:
                torch.where(over, rng_before, self.rng, out=self.rng)
                actions.masked_fill_(over, -1)
            probs = None
        if self.layout == 'tracked' and probs is None:
            # the hot call of a self-play loop: the env's own buffers are validated ONCE (gogame.batch_env_step_tracked's
            # checks, through _lib.ptrs), their pointers kept; a step is then the launch itself (8.6 -> 5.4 us of host time
            # per call).  Re-validated whenever one of the buffers is re-bound; they must not be resized in place.
            key = (id(self.tracked), id(self.rng), id(self._obs), id(self.steps_done), self.komi, self.reward_method, self.auto_reset)
            prep = self._prep
            if prep is None or prep[0] != key:
                # (the record keeps the tensors themselves: an object that is alive cannot hand its id() to a new one)
                prep = self._prep = (key, self._prepare_tracked_step(), (self.tracked, self.rng, self._obs, self.steps_done))
            fn, head, act, tail = prep[1]
            a = 0 if actions is None else _lib.dev_ptr(actions, act.kind, act.name)
            _lib.check(fn(head, a, *tail, _lib.stream_ptr(self.device)), _TRACKED_STEP)
            rewards, dones, status, taken = self._step_out
            self._obs_fresh = True
            if check and bool((status != 0).any()):
                raise AssertionError('illegal move in batch')
            return self._obs, rewards, dones, status
        if self.layout == 'tracked':
            rewards, dones, status, taken = gogame.batch_env_step_tracked(
                self.tracked, actions, self.rng, self.komi, self.reward_method, self.auto_reset, out=self._step_out,
                states_out=self._obs, steps_done=self.steps_done, weights=probs)   # the launch counts the played steps itself
            self._obs_fresh = True
            if check and bool((status != 0).any()):
                raise AssertionError('illegal move in batch')
            return self._obs, rewards, dones, status
        else:
            fn, store = ((gogame.batch_env_step_packed, self.packed_states) if self.packed
                         else (gogame.batch_env_step, self._states))
            rewards, dones, status, taken = fn(store, actions, self.rng, self.komi, self.reward_method, self.auto_reset,
                                               out=self._step_out)
            obs = store
        if check and bool((status != 0).any()):
            raise AssertionError('illegal move in batch')
        self.steps_done += (status == 0)
        return obs, rewards, dones, status

    def _prepare_tracked_step(self):
        """(entry point, first argument, the table's `actions` parameter, the arguments after it up to the stream) of
        gg_batch_env_step_tracked on this env's buffers, every tensor checked as gogame.batch_env_step_tracked checks it."""
        rewards, dones, status, taken = self._step_out
        B, N = self.batch_size, self.size
        if gogame._tracked_size(self.tracked) != N or self.tracked.shape[0] != B or tuple(self._obs.shape) != (B, 6, N, N):
            raise ValueError('the env\'s tracked boards / observation buffer do not have its batch and board size')
        for t, n in ((self.rng, B), (rewards, B), (dones, B), (status, B), (taken, B), (self.steps_done, B)):
            if t.numel() != n:
                raise ValueError('a step buffer of the env does not have one entry per game')
        head, *bufs = _lib.ptrs(_TRACKED_STEP, tracked=self.tracked, rng=self.rng, rewards=rewards, dones=dones, status=status,
                                taken_actions=taken, states_out=self._obs, steps_done=self.steps_done)
        tail = (*bufs, B, N, float(self.komi), gogame.REWARD_METHODS[self.reward_method], int(bool(self.auto_reset)))
        act = next(p for p in _lib.ABI[_TRACKED_STEP] if p.name == 'actions')
        return getattr(_lib.lib(), _TRACKED_STEP), head, act, tail

    def step_unfused(self, actions, check=False):
        """The same step as separate launches (reset, next_states, areas + torch reward arithmetic); float64 rewards."""
        if self.layout != 'bytes':
            raise NotImplementedError("step_unfused works on byte-plane states (layout='bytes')")
        if self.auto_reset:
            gogame.batch_reset_finished(self.states)
        actions = actions.to(device=self.device, dtype=torch.int32)
        self.states, status = gogame.batch_next_states(self.states, actions, check=False)
        if check and bool((status != 0).any()):
            raise AssertionError('illegal move in batch')
        self.last_actions.copy_(actions)
        self.steps_done += (status == 0).to(torch.int64)
        dones = self.states[:, govars.DONE_CHNL, 0, 0]   # planes 2/4/5 are uniform: one byte per game
        return self.states, self.rewards(dones), dones, status

    def rollout(self, plies):
        """`plies` uniform-random steps per game, fused on the device (boards stay on-chip).  Returns the RESIDENT store in
        its own layout (uint8 [B,6,N,N] for 'bytes', int32 [B,3N+1] for 'packed', int32 [B,5N+1] for 'tracked') - no
        conversion is run; read `env.states` for the uint8 observation (unlike step(), which always returns it)."""
        if self.layout == 'packed':
            gogame.batch_rollout_packed(self.packed_states, self.rng, plies, self.auto_reset, self.last_actions, self.steps_done)
            return self.packed_states
        if self.layout == 'tracked':
            gogame.batch_rollout_tracked(self.tracked, self.rng, plies, self.auto_reset, self.last_actions, self.steps_done)
            self._obs_fresh = False
            return self.tracked
        gogame.batch_rollout(self._states, self.rng, plies, self.auto_reset, self.last_actions, self.steps_done)
        return self._states

    def rewards(self, dones=None):
        """GoEnv.reward for every game (gym_go/envs/go_env.py:128-149), black's perspective."""
        black, white = gogame.batch_areas(self.states)
        margin = black.to(torch.float64) - white.to(torch.float64) - self.komi
        if dones is None:
            dones = self.states[:, govars.DONE_CHNL, 0, 0]
        over = dones.bool()
        if self.reward_method == 'real':
            return torch.where(over, torch.sign(margin), torch.zeros_like(margin))
        final = torch.where(margin > 0, 1.0, -1.0).to(torch.float64) * self.size ** 2
        return torch.where(over, final, margin)

    def turns(self):
        return self.states[:, govars.TURN_CHNL, 0, 0]


class GoVecEnvParts:
    """The games of a GoVecEnv as `parts` (default 2) sub-batches, each stepping on a HIP stream of its own.

    A step launch has a head (launch, board load, the ply: little memory traffic) and a tail (the observation
    write-back: nothing but memory traffic); one launch over the whole batch runs them one after the other on every CU at
    the same time.  Two half-batches that step independently put the head of one under the tail of the other
    (bench.py `gg_batch_env_step_two_half_batches_*`: 65 536 games of 19x19 step in 32 - 34 us instead of 38 - 39).  That is also
    the shape of a self-play loop: while the policy network evaluates one half's observation, the other half steps.

        env = GoVecEnvParts(65536, 19)
        env.step_part(0); env.step_part(1)                 # both halves in flight
        while True:
            for h in range(env.parts):
                obs, rewards, dones, status = env.wait(h)       # the caller's stream now sees part h's step
                probs = policy(obs)                             # caller's stream
                env.step_part(h, probs=probs)                   # queued behind `policy` on part h's stream

    The games are the games of ONE GoVecEnv(batch_size, ...): part h holds the games [first(h), first(h) + count(h)) of
    the contiguous split `shard` makes, seeded by their global index - stepping the parts in any interleaving walks the
    same games as the single env (tests/test_gpu_env.py).  Ordering: step_part(h) starts after everything queued so far on
    the caller's current stream (its inputs are ready, readers of part h's previous outputs are done) and after part h's
    own previous step; the tensors it returns are part h's fixed buffers, valid on the caller's stream after wait(h).
    Inside a hipGraph capture the parts' streams fork from and join the capturing stream (wait every part stepped
    before the capture ends)."""

    def __init__(self, batch_size, size, parts=2, first_game=0, device=None, **kwargs):
        if parts < 1 or parts > max(1, batch_size):
            raise ValueError('parts must be in [1, batch_size]')
        self.batch_size, self.size, self.parts = batch_size, size, parts
        self.device = torch.device(device) if device is not None else gogame._device()
        if self.device.type == 'cuda' and self.device.index is None:
            # an INDEXED device from here on: 'cuda' means "whatever is current NOW" - resolved again at every step it would
            # name another device's stream once the caller switches devices, while the kernels follow the tensors
            self.device = torch.device('cuda', torch.cuda.current_device())
        from gymgo_amd import _lib
        self._lib = _lib
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(parts)]
        self._raw = [s.cuda_stream for s in self.streams]
        self._hip = _lib.hip_runtime()
        # per part: "the caller's stream up to here" (fork) and "the part's last step" (done), re-recorded every step
        with torch.cuda.device(self.device):       # (an event belongs to the device that is current when it is created)
            self._fork = [_lib.hip_event() for _ in range(parts)]
            self._done = [_lib.hip_event() for _ in range(parts)]
        import ctypes
        self._cap = ctypes.c_int(0)
        self._cap_ref = ctypes.byref(self._cap)
        self.envs, self.bounds = [], []
        for h in range(parts):
            first, count = shard(batch_size, h, parts)
            self.bounds.append((first, first + count))
            # (the part's buffers are allocated on the part's stream: the caching allocator ties them to it)
            with torch.cuda.stream(self.streams[h]):
                self.envs.append(GoVecEnv(count, size, device=self.device, first_game=first_game + first, **kwargs))
        self._last = [None] * parts
        torch.cuda.current_stream(self.device).wait_stream(self.streams[-1])
        for s in self.streams[:-1]:
            torch.cuda.current_stream(self.device).wait_stream(s)

    def _capturing(self, raw):
        """Is `raw` being captured into a graph?  A failed query counts as "capturing": the event is then always recorded
        and the stream never queried - correct either way (hipStreamQuery on a capturing stream would invalidate the capture,
        and a stale answer of an earlier call must not be reused)."""
        self._cap.value = 1
        if self._hip.hipStreamIsCapturing(raw, self._cap_ref) != 0:
            return True
        return self._cap.value != 0

    def _fork_part(self, h):
        """Part h's stream waits for everything queued so far on the caller's current stream - unless that stream is
        idle (then everything on it HAS happened): an event pair per step is a marker in one hardware queue and a
        barrier in the other, microseconds of GPU time that would eat what the parts gain.  (Inside a stream capture
        the stream must not be queried: the fork is always recorded, it becomes an edge of the graph.)"""
        H, cur = self._hip, self._lib.current_raw_stream(self.device)
        if not self._capturing(cur) and H.hipStreamQuery(cur) == 0:
            return
        self._lib.check(H.hipEventRecord(self._fork[h], cur) or H.hipStreamWaitEvent(self._raw[h], self._fork[h], 0),
                        'GoVecEnvParts fork (hipEventRecord / hipStreamWaitEvent)')

    def step_part(self, h, actions=None, probs=None, check=False):
        """Queue GoVecEnv.step of part h on its stream, behind the caller's current stream.  Returns part h's
        (states, rewards, dones, status) buffers - read them after wait(h)."""
        env = self.envs[h]
        # conversions of the inputs (if any) are torch work on the CALLER's stream: done before the fork
        if actions is not None:
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if probs is not None:
            probs = gogame._weights_tensor(probs, env.batch_size, self.size, self.device)[0]
        self._fork_part(h)
        if env.layout == 'tracked' and not check:
            # no torch work inside this step (fixed buffers only): the launch is simply sent to the part's stream
            for t in (actions, probs):
                if t is not None and t.is_cuda:
                    t.record_stream(self.streams[h])
            with self._lib.stream_override(self._raw[h], self.device):
                self._last[h] = env.step(actions, probs=probs)
        else:
            for t in (actions, probs):
                if t is not None and t.is_cuda:
                    t.record_stream(self.streams[h])
            with torch.cuda.stream(self.streams[h]):
                self._last[h] = env.step(actions, check=check, probs=probs)
        return self._last[h]

    def wait(self, h):
        """The caller's current stream waits for everything queued on part h's stream - its last step; returns that
        step's buffers (None before the first).  (The event is recorded here, not by the step: a loop that never waits
        puts no markers between its launches.)"""
        H, cur = self._hip, self._lib.current_raw_stream(self.device)
        if not self._capturing(cur) and H.hipStreamQuery(self._raw[h]) == 0:
            return self._last[h]            # the part has finished: there is nothing left to order
        self._lib.check(H.hipEventRecord(self._done[h], self._raw[h]) or H.hipStreamWaitEvent(cur, self._done[h], 0),
                        'GoVecEnvParts wait (hipEventRecord / hipStreamWaitEvent)')
        return self._last[h]

    def ready(self, h):
        """True when everything queued on part h's stream has finished (a host-side poll, no synchronisation).  Inside a
        stream capture nothing has run yet and a query would invalidate the capture: False without asking."""
        if self._capturing(self._lib.current_raw_stream(self.device)) or self._capturing(self._raw[h]):
            return False
        return self._hip.hipStreamQuery(self._raw[h]) == 0

    def step(self, actions=None, probs=None, check=False):
        """Every part steps (actions / probs are split along the game axis), the caller's stream waits for all of them:
        the lock-step form, for code that wants one call - the overlap between parts is then limited to this one step."""
        outs = []
        for h, (lo, hi) in enumerate(self.bounds):
            self.step_part(h, None if actions is None else actions[lo:hi], None if probs is None else probs[lo:hi], check)
        for h in range(self.parts):
            outs.append(self.wait(h))
        return outs

    def rollout_part(self, h, plies):
        self._fork_part(h)
        with torch.cuda.stream(self.streams[h]):
            out = self.envs[h].rollout(plies)
        return out

    def __del__(self):
        try:
            for ev in self._fork + self._done:
                self._hip.hipEventDestroy(ev)
        except Exception:
            pass

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def gather(self, name):
        """torch.cat of an attribute of the parts (`states`, `rng`, `steps_done`, `last_actions`, `tracked` ...), on the
        caller's stream after waiting for every part."""
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)
        return torch.cat([getattr(e, name) for e in self.envs])
