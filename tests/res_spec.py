"""An independent, literal specification of one spatial resource step.

A plain, slow restatement of one pass of the reference's DoSpatialUpdates
loop body for ONE resource (main/cResourceCount.cc:830-846): Source, Sink,
CellInflow + CellOutflow (only with a CELL list), FlowAll, StateAll, written
from the reference's sources main/cSpatialResCount.cc (SetPointers, Source,
Sink, CellInflow, CellOutflow, FlowAll, StateAll) and main/cResourceCount.cc
(FlowMatter) -- not from oracle/oracle.cc and not from resources.hip, which
both reach a neighbour by arithmetic on (x, y).  Here the eight-pointer table
is built per cell as SetPointers builds it (all cells as a torus, then the
GRID fix-ups in its order) and FlowAll walks `for i ... for k = 3..6` over
that table.

Python floats are IEEE doubles and nothing contracts; every division is a
real division as FlowMatter writes it (/ 16.0, / 3.0, / (|xdist| + |ydist|),
/ dist with dist = math.sqrt(2.0) or 1.0).

The inflow / outflow boxes are used RAW: cSpatialResCount::CheckRanges, which
would clamp them into the world, is dead code in the reference -- nothing
calls it -- so a coordinate of cResource::NONE (-99), a box that exceeds the
world and an inverted box all reach Source and Sink as written in the
environment file.

Besides the new amounts a step can fill a Counts: how often the operand of
one of FlowMatter's divisions by a non-power-of-two (x / 3.0, x / sqrt(2)) was
zero, inside [2^-900, 2^900] or outside it -- the three classes the device's
reciprocal correction tells apart -- with the zero operands counted once more
where the gravity constant is not zero or the flow is diagonal (zero_live:
with zero gravity x is the signed zero -a2 * 0 whatever the amounts, and the
device folds that division away; the operands below 2^-900 of those live
divisions are kept, in Counts.tiny), how many flows ran between equal amounts,
and how often Source covered each cell.  The tests assert on those, so that
no case passes without reaching the paths it is there for.
"""
import math

NONE = -99                      # cResource::NONE
GRID, TORUS = 1, 2              # nGeometry::GRID / TORUS as the C ABI numbers them
SQRT2 = math.sqrt(2.0)
LO, HI = 2.0 ** -900, 2.0 ** 900


def mod(value, base):
    """AvidaTools::Mod: C's truncating %, then lifted into [0, base)"""
    value = int(math.fmod(value, base))
    return value + base if value < 0 else value


def grid_neighbor(cell_id, size_x, size_y, diff_x, diff_y):
    """AvidaTools::GridNeighbor"""
    new_x = mod((cell_id % size_x) + diff_x, size_x)
    new_y = mod((cell_id // size_x) + diff_y, size_y)
    return new_y * size_x + new_x


def set_pointers(geometry, world_x, world_y):
    """cSpatialResCount::SetPointers: per cell eight [elem, xdist, ydist, dist],
    pointer 0 up-left and clockwise from there"""
    num_cells = world_x * world_y
    offs = [(-1, -1, SQRT2), (0, -1, 1.0), (+1, -1, SQRT2), (+1, 0, 1.0),
            (+1, +1, SQRT2), (0, +1, 1.0), (-1, +1, SQRT2), (-1, 0, 1.0)]
    grid = []
    for i in range(num_cells):                       # first all cells as in a torus
        grid.append([[grid_neighbor(i, world_x, world_y, dx, dy), dx, dy, dist] for dx, dy, dist in offs])
    none = [NONE, NONE, NONE, NONE]
    if geometry == GRID:
        for i in range(world_x):                     # top and bottom
            for k in (0, 1, 2):
                grid[i][k] = list(none)
            ii = num_cells - 1 - i
            for k in (4, 5, 6):
                grid[ii][k] = list(none)
        for i in range(world_y):                     # left and right sides
            ii = i * world_x
            for k in (0, 7, 6):
                grid[ii][k] = list(none)
            ii = ((i + 1) * world_x) - 1
            for k in (2, 3, 4):
                grid[ii][k] = list(none)
    return grid


class Counts:
    """what a run of steps went through (see the module docstring)"""

    def __init__(self):
        self.zero = self.inside = self.outside = 0
        self.zero_live = 0      # zero operands of a division the device does not fold away
        self.equal_ends = 0
        self.cover = None       # Source's visits per cell in the last step
        self.finite = True
        self.tiny = []          # (x, divisor) of the live operands below 2^-900

    def operand(self, x, live, c):
        ax = abs(x)
        if live and 0.0 < ax < LO:
            self.tiny.append((x, c))
        if ax == 0.0:
            self.zero += 1
            self.zero_live += live
        elif LO <= ax <= HI:
            self.inside += 1
        else:
            self.outside += 1


def _div(a, b):
    """a / b as IEEE does it when b is zero (Source's share of an empty box);
    everywhere else Python's own division"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def flow_matter(amount, delta, e1, e2, inxdiffuse, inydiffuse, inxgravity, inygravity, xdist, ydist, dist,
                counts=None):
    """FlowMatter (main/cResourceCount.cc:40-98) between elements e1 and e2"""
    if amount[e1] == 0.0 and amount[e2] == 0.0 and dist < 0.0:
        return
    diff = amount[e1] - amount[e2]
    if counts is not None and amount[e1] == amount[e2]:
        counts.equal_ends += 1
    if xdist != 0:
        if (xdist > 0 and inxgravity > 0.0) or (xdist < 0 and inxgravity < 0.0):
            num = amount[e1] * math.fabs(inxgravity)
        else:
            num = -amount[e2] * math.fabs(inxgravity)
        if counts is not None:
            counts.operand(num, inxgravity != 0.0, 3.0)
        xgravity = num / 3.0
        xdiffuse = inxdiffuse * diff / 16.0
    else:
        xdiffuse = 0.0
        xgravity = 0.0
    if ydist != 0:
        if (ydist > 0 and inygravity > 0.0) or (ydist < 0 and inygravity < 0.0):
            num = amount[e1] * math.fabs(inygravity)
        else:
            num = -amount[e2] * math.fabs(inygravity)
        if counts is not None:
            counts.operand(num, inygravity != 0.0, 3.0)
        ygravity = num / 3.0
        ydiffuse = inydiffuse * diff / 16.0
    else:
        ydiffuse = 0.0
        ygravity = 0.0
    q = (xdiffuse + ydiffuse + xgravity + ygravity) / (math.fabs(xdist * 1.0) + math.fabs(ydist * 1.0))
    if counts is not None and dist != 1.0:
        counts.operand(q, True, dist)
    flowamt = q / dist
    delta[e1] -= flowamt
    delta[e2] += flowamt


def step(params, cells, X, Y, amounts, counts=None):
    """One DoSpatialUpdates pass over one resource.

    params: an object with the fields of files.Resource (geometry 1 / 2,
    inflow, outflow, the raw boxes, x/ydiffuse, x/ygravity); cells: this
    resource's CELL entries in list order (objects with .cell, .inflow,
    .outflow); amounts: X * Y doubles.  Returns the new amounts (a list)."""
    p = params
    num_cells = X * Y
    amount = [float(a) for a in amounts]
    delta = [0.0] * num_cells
    grid = set_pointers(p.geometry, X, Y)

    # Source(inflow_rate)
    totalcells = (p.inflow_y2 - p.inflow_y1 + 1) * (p.inflow_x2 - p.inflow_x1 + 1) * 1.0
    share = _div(p.inflow, totalcells)
    cover = [0] * num_cells
    for i in range(p.inflow_y1, p.inflow_y2 + 1):
        for j in range(p.inflow_x1, p.inflow_x2 + 1):
            elem = mod(i, Y) * X + mod(j, X)
            delta[elem] += share
            cover[elem] += 1

    # Sink(decay_rate), decay_rate = 1 - outflow (cPopulation.cc sets it so)
    decay = 1.0 - p.outflow
    if not (p.outflow_x1 == NONE or p.outflow_y1 == NONE or p.outflow_x2 == NONE or p.outflow_y2 == NONE):
        for i in range(p.outflow_y1, p.outflow_y2 + 1):
            for j in range(p.outflow_x1, p.outflow_x2 + 1):
                elem = mod(i, Y) * X + mod(j, X)
                v = amount[elem] * (1.0 - decay)
                deltaamount = v if v > 0.0 else 0.0          # Apto::Max(v, 0.0)
                delta[elem] += -deltaamount

    if len(cells) > 0:
        # CellInflow
        for c in cells:
            if 0 <= c.cell < num_cells:
                delta[c.cell] += c.inflow
        # CellOutflow: Rate() is called for every entry, but does nothing for
        # an id outside the grid (its assert is compiled out)
        deltaamount = 0.0
        for c in cells:
            if 0 <= c.cell < num_cells:
                v = amount[c.cell] * c.outflow
                deltaamount = v if v > 0.0 else 0.0
            if 0 <= c.cell < num_cells:
                delta[c.cell] += -deltaamount

    # FlowAll
    if not (p.xdiffuse == 0.0 and p.ydiffuse == 0.0 and p.xgravity == 0.0 and p.ygravity == 0.0):
        for i in range(num_cells):
            for k in range(3, 7):
                ii, xdist, ydist, dist = grid[i][k]
                if ii >= 0:
                    flow_matter(amount, delta, i, ii, p.xdiffuse, p.ydiffuse, p.xgravity, p.ygravity,
                                xdist, ydist, dist, counts)

    # StateAll
    for i in range(num_cells):
        amount[i] += delta[i]
    if counts is not None:
        counts.cover = cover
        counts.finite = counts.finite and all(math.isfinite(a) for a in amount)
    return amount


def level(amounts):
    """a resource's level as avgpu_get_resources reports it: the cells summed
    in index order (cSpatialResCount::SumAll)"""
    s = 0.0
    for a in amounts:
        s += a
    return s
