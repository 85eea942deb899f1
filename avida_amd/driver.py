"""Avida2Driver restated over the C-ABI (targets/avida/Avida2Driver.cc:91-163).

Reads a reference config directory (avida.cfg, the instruction set, the
environment file with REACTION / RESOURCE / CELL lines, events.cfg), runs the
world on the MI355X path (`libavida_gpu.so`) and writes the reference's data
files (avida_amd/datafiles.py).  The update loop keeps the reference's event
timing: "begin" events run before update 0; an event of update u runs after
update u has been processed (the next iteration's GetEvents), so a print at u
shows the state at the end of update u, and "u N Exit" ends after update N.

Events on this path (main/cEventList.cc syntax "u <start>[:<interval>[:<end>]]"):
Inject <org> [cell] [merit], InjectAll <org> [merit], InjectSequence <seq>
[start] [end] [merit], LoadPopulation <file> [update] [cellid_offset] (.pop /
.spop, avida_amd/population.py), SavePopulation [name] (<name>-<update>.spop),
Print{Count,Average,Tasks,Time,Resource,Dominant}Data [file],
PrintGeneticDistanceData <ref.org> [file], PrintPopulationDistanceData
<ref.org> [file], CalcConsensus [lines_saved] (avida_amd/distance.py; the .org
path is relative to the config directory), SaveCheckpoint [file] /
LoadCheckpoint <file> (full hardware state, avida_amd/checkpoint.py;
after LoadCheckpoint the driver's update counter is the checkpoint's, so the
next update processed is the one after it and later events fire by that
numbering, as LoadPopulation's update argument does), the population events
of avida_amd/popevents.py -- KillProb / KillRate [p = 0.9], KillRectangle
[x1 y1 x2 y2 = 0], ApplyBottleneck [size = 100], SerialTransfer [size = 1]
[ignore_deads = 1], KillDominantGenotype, KillProbSequence <sequence>
[p = 0.9]; each draws with the key (update << 32) | index of its line among
the events -- and Exit.  Other Print* events write nothing; anything else is
an error.

    python -m avida_amd.driver -c <config dir> -d <data dir> [-u MAX_UPDATES]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

from . import capi, datafiles, distance, files, popevents, population, systematics
from .world import World


class ProductWorld(World):
    """The world on the GPU through libavida_gpu.so: world.World plus what
    only the product has (the driver runs on either; a world without these
    methods takes the host route)."""

    def __init__(self, cfg, iset, env, ncells=0, device=0, serial=False):
        super().__init__(cfg, iset, env, ncells, device)
        self.serial = serial       # every update under the reference's own schedule (World.run_update)

    def run_update(self):
        return super().run_update(self.serial)

    def test_genomes(self, genomes, flags_cap=2049):
        return super().test_genomes(genomes, flags_cap, offspring=False)

    def resources(self, spatial=False):
        return super().resources(False)          # the levels alone: (levels, None)

    def parent_keys(self, first=0, count=None):
        """each cell's organism's parent's genotype key, 0 for an injected
        organism or a dead cell (avgpu_get_parent_keys)"""
        import numpy as np
        out = np.zeros(self.ncells - first if count is None else count, dtype=np.uint64)
        self._call("get_parent_keys", self.h, first, len(out), out.ctypes.data_as(C.c_void_p))
        return out

    def genotypes(self):
        """(table, totals): the census grouped by key on the device
        (avgpu_get_genotypes)"""
        return capi.get_genotypes(self.lib, self.h)

    def classify_genotypes(self, update, threshold):
        """one classification by the arbiter kept on the device
        (avgpu_classify_genotypes): its summary record"""
        return capi.classify_genotypes(self.lib, self.h, update, threshold)

    def enable_lineage(self, on=True, rows_hint=0, arena_hint=0):
        capi.enable_lineage(self.lib, self.h, on, rows_hint, arena_hint)

    def lineage_state(self, summary_only=False):
        """(rows, arena, summary) of the device lineage store (avgpu_get_lineage)"""
        return capi.get_lineage(self.lib, self.h, summary_only)

    def prune_lineage(self):
        return capi.prune_lineage(self.lib, self.h)

    def arbiter_state(self):
        """(rows, table, summary, sz_count) of the last classification
        (avgpu_get_arbiter)"""
        return capi.get_arbiter(self.lib, self.h)

    def landscape(self, genomes, distance=1, chart=None):
        """the full substitution landscapes of `genomes` on the device
        (avgpu_landscapes): a list of landscape.Landscape"""
        from . import landscape
        return landscape.full(self, genomes, distance, chart)

    def pair_distances(self, genomes, pairs):
        """(hamming, edit) of pairs of genomes on the device (avgpu_genome_distances)"""
        return distance.pair_distances(self, genomes, pairs)

    def cell_distances(self, ref, first=0, count=None):
        """(hamming, edit) of every cell's organism to the genome `ref`, -1
        for an empty cell (avgpu_cell_distances)"""
        return distance.cell_distances(self, ref, first, count)

    def site_histogram(self, first=0, count=None):
        """(hist, num_living): CalcConsensus' per-site instruction histogram
        of the living organisms (avgpu_site_histogram)"""
        return distance.site_histogram(self, first, count)

    def kill_cells(self, cells):
        """kill the listed cells on the device (avgpu_kill_cells); like the
        four below it returns the living organisms killed"""
        return popevents.kill_cells(self, cells)

    def kill_prob(self, p, key):
        """every organism dies with probability p (avgpu_kill_prob; KillProb)"""
        return popevents.apply_kill_prob(self, p, key)

    def kill_rect(self, x1=0, y1=0, x2=0, y2=0):
        """KillRectangle's raw arguments (avgpu_kill_rect)"""
        return popevents.apply_kill_rect(self, x1, y1, x2, y2)

    def kill_genotypes(self, keys, p, key):
        """the organisms of the listed genotype keys die with probability p (avgpu_kill_genotypes)"""
        return popevents.apply_kill_genotypes(self, keys, p, key)

    def keep_sample(self, keep, key):
        """a uniform sample of `keep` organisms survives (avgpu_keep_sample;
        SerialTransfer, ApplyBottleneck)"""
        return popevents.apply_keep_sample(self, keep, key)


def load_config(config_dir):
    """(avida config, instruction set, environment, events) of a reference config dir"""
    cfg = files.read_avida_cfg(os.path.join(config_dir, "avida.cfg"))
    iset = cfg.instset
    if iset is None:
        name = cfg.get("INST_SET", "-")
        path = os.path.join(config_dir, name if name not in ("-", "") else "instset-heads.cfg")
        iset = files.read_instset(path)
    env = files.read_environment(os.path.join(config_dir, cfg.get("ENVIRONMENT_FILE", "environment.cfg")))
    events = files.read_events(os.path.join(config_dir, cfg.get("EVENT_FILE", "events.cfg")))
    return cfg, iset, env, events


def _fires(trigger, start, u):
    """does an update event "u <start>[:<interval>[:<end>]]" fire after update u?"""
    if trigger != "u":
        raise ValueError(f"event trigger {trigger!r} is not supported on this path")
    parts = start.split(":")
    if parts[0] == "begin":
        return False
    s = int(parts[0])
    if len(parts) == 1:
        return u == s
    step = int(parts[1])
    end = parts[2] if len(parts) > 2 else "end"
    if u < s or (end != "end" and u > int(end)):
        return False
    return (u - s) % step == 0


class Driver:
    def __init__(self, config_dir, data_dir, make_world=None, seed=None, lineage=False):
        self.config_dir = config_dir
        acfg, self.iset, self.env, self.events = load_config(config_dir)
        self.cfg = capi.cfg_from_avida(acfg, seed=seed)
        self.world = (make_world or ProductWorld)(self.cfg, self.iset, self.env)
        self.rec = datafiles.StatsRecorder(data_dir, [r.name for r in getattr(self.env, "resources", [])])
        self.data_dir = data_dir
        # genotype classification runs every update when a data file needs it
        # (the reference's systematics manager classifies every birth)
        need = {"PrintCountData", "PrintDominantData", "SavePopulation", "PrintAverageData", *distance.Actions.NAMES,
                "KillDominantGenotype"}
        # (on the device where the world keeps the arbiter there, else on the host)
        kind = systematics.DeviceGenotypeArbiter if hasattr(self.world, "classify_genotypes") \
            else systematics.GenotypeArbiter
        self.arbiter = kind(int(acfg.get("THRESHOLD", 3))) if any(e[2] in need for e in self.events) else None
        # lineage=True: ancestry (parents, depth, lineages) in the store
        # the device keeps beside its arbiter
        self.lineage = bool(lineage)
        if self.lineage:
            if not hasattr(self.world, "parent_keys") or not hasattr(self.world, "enable_lineage"):
                raise ValueError(f"lineage=True needs a world that records parent keys; "
                                 f"{type(self.world).__name__} has none")
            self.arbiter = systematics.DeviceGenotypeArbiter(int(acfg.get("THRESHOLD", 3)), lineage=True)
            self.arbiter.enable(self.world)
        self.rec.arbiter = self.arbiter
        # the genetic-distance actions (avida_amd/distance.py): on the device where the world answers there
        self.dist = distance.Actions(self.world, self.iset, data_dir, config_dir)
        self.done = False
        self.update = -1
        self.event_index = 0          # the line, among the events, of the event being run
        self.unsequenced = 0          # genotypes SerialTransfer's "ignore deads" left alone (_population_event)

    def _org(self, name):
        return files.read_org(os.path.join(self.config_dir, name), self.iset)

    def _classify(self):
        """the arbiter takes the world's genotype table: the device's where
        the world has one, else the census grouped on the host; a world that
        keeps the arbiter on the device classifies there"""
        w = self.world
        if isinstance(self.arbiter, systematics.DeviceGenotypeArbiter):
            self.arbiter.classify(w, max(self.update, 0))
            return
        table, totals = w.genotypes() if hasattr(w, "genotypes") else systematics.table_from_census(w.census())
        self.arbiter.update_table(table, totals, max(self.update, 0))

    POPULATION_EVENTS = ("KillProb", "KillRate", "KillRectangle", "ApplyBottleneck", "SerialTransfer",
                         "KillDominantGenotype", "KillProbSequence")

    def _population_event(self, action, args):
        """The population actions of actions/PopulationActions.cc through
        avida_amd/popevents.py: on the device where the world decides them
        there, else from the census, cell by cell.  The event's draws are keyed
        by (update << 32) | index of its line among the events.
        SerialTransfer with ignore_deads first kills the genotypes whose test
        fitness is 0 (cPopulation::SerialTransfer, main/cPopulation.cc:
        7559-7564), from the sequences of the living genotypes obtained as
        population.save_population obtains them; a genotype without a sequence
        (every member has copied into its own first sites) is left alone, and
        self.unsequenced counts them."""
        w = self.world
        key = (max(self.update, 0) << 32) | self.event_index
        if action in ("KillProb", "KillRate"):               # :1171-1175; KillRate is its alias (:5743)
            popevents.apply_kill_prob(w, float(args[0]) if args else 0.9, key)
        elif action == "KillRectangle":                      # :1762-1768
            popevents.apply_kill_rect(w, *[int(a) for a in args[:4]])
        elif action == "ApplyBottleneck":                    # :1200-1204 (a negative size never ends there)
            popevents.apply_keep_sample(w, max(int(args[0]) if args else 100, 0), key)
        elif action == "SerialTransfer":                     # :1839-1846
            size = int(args[0]) if args else 1
            ignore_deads = int(args[1]) if len(args) > 1 else 1
            if size < 0:
                size = 1
            if ignore_deads:
                dead, unsequenced = popevents.dead_genotype_keys(w, self.iset)
                self.unsequenced += unsequenced
                popevents.apply_kill_genotypes(w, dead, 1.0, key)
            popevents.apply_keep_sample(w, size, key)
        elif action == "KillDominantGenotype":               # :1240-1256
            best = self.arbiter.best_key
            if best is not None:
                popevents.apply_kill_genotypes(w, [int(best)], 1.0, key)
        elif action == "KillProbSequence":                   # :1268-1273
            genome = self.iset.parse_sequence(args[0])
            gkey = systematics.genome_key(bytes(self.iset.handlers[x] for x in genome))
            popevents.apply_kill_genotypes(w, [gkey], float(args[1]) if len(args) > 1 else 0.9, key)
        if self.arbiter is not None:          # the survivors are classified at once, as after injections
            self._classify()

    def _action(self, action, args):
        w = self.world
        if action in self.POPULATION_EVENTS:
            self._population_event(action, args)
            return
        if action == "Inject":
            cell = int(args[1]) if len(args) > 1 else 0
            merit = float(args[2]) if len(args) > 2 else -1.0
            w.set_orgs(cell, [self._org(args[0])], [max(0.0, merit)], deterministic=False)
            self.rec.injected += 1
        elif action == "InjectAll":
            g = self._org(args[0])
            merit = float(args[1]) if len(args) > 1 else -1.0
            n = self.cfg.world_x * self.cfg.world_y
            w.set_orgs(0, [g] * n, [max(0.0, merit)] * n, deterministic=False)
            self.rec.injected += n
        elif action.lower() == "injectsequence":
            g = self.iset.parse_sequence(args[0])
            start = int(args[1]) if len(args) > 1 else 0
            end = int(args[2]) if len(args) > 2 else start + 1
            merit = float(args[3]) if len(args) > 3 else -1.0
            w.set_orgs(start, [g] * (end - start), [max(0.0, merit)] * (end - start), deterministic=False)
            self.rec.injected += end - start
        if action in ("Inject", "InjectAll") or action.lower() == "injectsequence":
            if self.arbiter is not None:      # injected units are classified at once
                self._classify()
            return
        if action == "PrintCountData":
            self.rec.print_count(*args[:1])
        elif action == "PrintDominantData":
            self.rec.print_dominant(*args[:1])
        elif action == "PrintAverageData":
            self.rec.print_average(*args[:1])
        elif action == "PrintTasksData":
            self.rec.print_tasks(*args[:1])
        elif action == "PrintTimeData":
            self.rec.print_time(*args[:1])
        elif action == "PrintResourceData":
            self.rec.print_resource(w.resources()[0], *args[:1])
        elif action == "SavePopulation":          # actions/SaveLoadActions.cc:168-176
            name = args[0] if args else "detail"
            historic = int(args[1]) != 0 if len(args) > 1 else True      # save_historic (SaveLoadActions.cc:142)
            if self.lineage and historic:
                self.arbiter.prune()                # the historic rows written: the living genotypes' ancestors
            population.save_population(w, self.iset, self.arbiter,
                                       os.path.join(self.data_dir, f"{name}-{max(self.update, 0)}.spop"),
                                       max(self.update, 0),
                                       lineage=self.arbiter.lineage_store() if self.lineage and historic else None)
        elif action == "LoadPopulation":          # actions/SaveLoadActions.cc:62-88
            if len(args) > 1 and int(args[1]) >= 0:
                self.update = int(args[1]) - 1     # SetCurrentUpdate: the next update is that one
            offset = int(args[2]) if len(args) > 2 else 0
            self.rec.injected += population.load_population(
                w, self.iset, os.path.join(self.config_dir, args[0]), w.ncells, offset)
            if self.arbiter is not None:
                self._classify()
        elif action == "SaveCheckpoint":
            name = args[0] if args else f"checkpoint-{self.update}.npz"
            w.checkpoint(os.path.join(self.data_dir, name))
        elif action == "LoadCheckpoint":
            stats = w.restore(os.path.join(self.config_dir, args[0]))
            self.rec.end_update(stats)
            self.update = int(stats.update)          # the next update is the one after the checkpoint's
            if isinstance(self.arbiter, systematics.DeviceGenotypeArbiter):
                self.arbiter.attach(w)               # the checkpoint carried the arbiter's state
        elif action in distance.Actions.NAMES:
            self.dist.run(action, args, self.arbiter, max(self.update, 0))
        elif action == "Exit":
            self.done = True
        elif action.startswith("Print"):
            pass   # data outside this path (genotypes, systematics ...): not written
        else:
            raise ValueError(f"event action {action!r} is not supported on this path")

    def run(self, max_updates=None):
        for i, (trig, start, action, args) in enumerate(self.events):
            if start.split(":")[0] == "begin":
                self.event_index = i
                self._action(action, args)
        while not self.done and (max_updates is None or self.update + 1 < max_updates):
            self.update += 1
            if self.update > 0:
                self.rec.begin_update()
            self.rec.end_update(self.world.run_update())
            if self.arbiter is not None:
                self._classify()
            for i, (trig, start, action, args) in enumerate(self.events):
                if _fires(trig, start, self.update):
                    self.event_index = i
                    self._action(action, args)
        self.rec.close()
        self.dist.close()
        return self.update


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-c", "--config", default=".")
    ap.add_argument("-d", "--data", default="data")
    ap.add_argument("-u", "--max-updates", type=int, default=None)
    ap.add_argument("-s", "--seed", type=int, default=None)
    ap.add_argument("--serial", action="store_true",
                    help="the reference's own per-step schedule (avgpu_run_serial_updates) "
                         "instead of the batch update")
    a = ap.parse_args(argv)
    mk = (lambda cfg, iset, env: ProductWorld(cfg, iset, env, serial=True)) if a.serial else None
    d = Driver(a.config, a.data, make_world=mk, seed=a.seed)
    last = d.run(a.max_updates)
    print(f"ran updates 0..{last}", file=sys.stderr)
    d.world.close()


if __name__ == "__main__":
    main()
