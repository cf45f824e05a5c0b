"""The graph-length rule of the sampler loops (ldc_graph_schedule), restated in Python from the rule as the header
documents it: a loop of n_steps steps over `parts` batch parts replays captured graphs of K steps, and graphs of one step for the rest.

  want   the "graph_steps" option when it is set; else 5 steps per graph for a strided loop (DDIM, DPM) or for several parts, 10 for the
         single chain of a DDPM loop (about 1 500 kernel nodes per graph either way).
  DDPM, option unset: a remainder of one-step replays is slow, so a length that divides n_steps is preferred -- among the divisors in the
         flat part of the measured range (8..25 for one part, 3..7 for several) the one nearest to want, the smaller of two equally near.
  K      want for a strided loop, so that every step count replays the same graphs; else want clamped to n_steps - 1 (the loop that
         captures has run one step eagerly), and never below 1.
"""
MAX_PARTS = 4
DIVISOR_RANGE = {True: range(8, 26), False: range(3, 8)}          # keyed by "one part"


def schedule(n_steps, parts, strided, option):
    """-> (K, n_big, n_single): n_big replays of the K-step graph and n_single of the one-step graph make n_steps steps"""
    if n_steps < 1 or not 1 <= parts <= MAX_PARTS or option < 0:
        raise ValueError((n_steps, parts, option))
    if option > 0:
        want = option
    else:
        want = 10 if parts == 1 and not strided else 5
        if not strided:
            divisors = [k for k in DIVISOR_RANGE[parts == 1] if n_steps % k == 0]
            if divisors:
                want = min(divisors, key=lambda k: (abs(k - want), k))
    K = want if strided else max(1, min(want, n_steps - 1))
    n_big, n_single = divmod(n_steps, K)
    return K, n_big, n_single


def launches(n_steps, parts, strided, option, per_part, captures=False):
    """graph launches of one loop: every replay is one launch per part on per-part graphs, one launch on the fork / join graph.  A loop
    that captures runs its first step eagerly and replays the rest with the K of the whole loop."""
    K, n_big, n_single = schedule(n_steps, parts, strided, option)
    if captures:
        n_big, n_single = divmod(n_steps - 1, K)
    return (parts if per_part else 1) * (n_big + n_single)
