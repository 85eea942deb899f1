"""Time the device population events on the bench world against the host route
they replace (measurement only).

The world is bench.py's (its build_world: 1024 x 1024 cells seeded from
detail-50000.pop, 150 burn-in updates).  On one device in one session, each
case on a world of its own as the burn-in leaves it:

* avgpu_kill_prob(0.5), avgpu_keep_sample(1000) and avgpu_kill_rect over a
  quarter of the world: device ms (HIP events, avgpu_last_event_ms), the
  control words read, wall ms of the call with the count returned, and the
  organisms killed -- after one warm-up call on a scratch state;
* the host route: avgpu_kill over 4096 living cells, wall ms, and that figure
  times victims / 4096, EXTRAPOLATED to each case's victim count and labelled
  so.

    python tools/events_timing.py [--out profiles/pop_events_timing.txt] [--side 1024]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_KILLS = 4096


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--burn-in", type=int, default=None)
    ap.add_argument("--seed", type=int, default=101)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import numpy as np
    import bench
    from avida_amd import capi, files, popevents
    lib = capi.load_product()
    golden = os.path.join(ROOT, "tests", "golden")
    burn = bench.BURN_IN if a.burn_in is None else a.burn_in

    class World:                                  # what avida_amd.popevents asks of a world
        p = "avgpu_"

        @staticmethod
        def census():
            return capi.get_census(lib, "avgpu_", World.h, 0, World.ncells)
    World.lib = lib

    def burnt_in():
        """bench.py's world after its burn-in, as World"""
        World.h, World.cfg, World.ncells, _ = bench.build_world(lib, capi, files, golden, a.side, a.seed, 0, 0, 1)
        for _ in range(burn):
            capi.check(lib, lib.avgpu_run_update(World.h, None))
        capi.check(lib, lib.avgpu_sync(World.h))

    side = a.side
    key = (burn << 32) | 1
    cases = [("kill_prob(0.5)", lambda: popevents.apply_kill_prob(World, 0.5, key)),
             ("keep_sample(1000)", lambda: popevents.apply_keep_sample(World, 1000, key)),
             ("kill_rect(quarter)", lambda: popevents.apply_kill_rect(World, 0, 0, side // 2 - 1, side // 2 - 1))]
    lines, results = [], []
    for i, (name, call) in enumerate(cases):          # every case on the world as the burn-in leaves it
        if i:
            lib.avgpu_destroy(World.h)
        burnt_in()
        if not i:
            living = int(popevents.alive_mask(World)[0].sum())
            lines += [f"# bench world {side} x {side}, {burn} burn-in updates: {living} organisms in {World.ncells} cells",
                      "# case killed words_read device_ms call_wall_ms"]
        popevents.apply_kill_prob(World, 0.0, 0)      # warm-up calls: the scratch exists, nobody dies
        popevents.apply_keep_sample(World, 1 << 40, 0)
        t0 = time.perf_counter()
        killed = call()
        wall = (time.perf_counter() - t0) * 1e3
        ms, words = popevents.last_timing(World)
        results.append((name, killed))
        lines.append(f"{name} {killed} {words} {ms:.4f} {wall:.3f}")
        print(lines[-1], flush=True)
    # the host route on the last world: avgpu_kill over 4096 of the survivors
    alive, _ = popevents.alive_mask(World)
    victims = np.flatnonzero(alive)[:HOST_KILLS]
    t0 = time.perf_counter()
    for c in victims.tolist():
        capi.check(lib, lib.avgpu_kill(World.h, c))
    host_ms = (time.perf_counter() - t0) * 1e3
    lines += [f"# host route: avgpu_kill over {len(victims)} living cells, wall ms, and x victims / {len(victims)} "
              f"EXTRAPOLATED to each case's victims",
              "# case host_kills host_wall_ms extrapolated_ms",
              f"avgpu_kill {len(victims)} {host_ms:.1f} -"]
    for name, killed in results:
        lines.append(f"{name} {killed} - {host_ms * killed / max(1, len(victims)):.0f}")
    lib.avgpu_destroy(World.h)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
