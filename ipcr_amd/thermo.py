"""Host side of `ipcr-thermo --thermo-model legacy-heuristic`: solution conditions, the perfect-duplex Tm behind `--denom
auto`, the score ordering and Go's float formats.  The score itself is computed by the library: per product on the device
(ipcr_thermo_legacy_products), per end on the host (ipcr_thermo_legacy_penalty).

Restates core/thermo/conditions.go, core/thermo/nn.go:94-301, internal/thermovisitors/score.go:95-110 and :465-492, and
internal/common/sort.go:81-95.  Of the NN models nn-duplex-v1 is built as a library feature: PerfectDuplex and panel_nn_base
give the per-primer base that ipcr_thermo_nn_duplex_products takes (engine.SimulationScratch.thermo_nn_scores); the driver
still refuses the model (UNBUILT_MODELS), and nn-structure-v1 is not built.
"""
from __future__ import annotations

import ctypes as C
import math
import re
from dataclasses import dataclass, replace
from typing import Optional, Sequence

from . import _lib

LEGACY_HEURISTIC = "legacy-heuristic"
UNBUILT_MODELS = ("nn-duplex-v1", "nn-structure-v1")        # internal/thermomodel: the reference's default is the second
FIXED_DENOM = 200.0
RCAL = 1.9872                                               # gas constant, cal/(K mol)

SALT_MONOVALENT, SALT_OWCZARZY_LITE, SALT_OWCZARZY08 = "monovalent", "owczarzy-lite", "owczarzy08"
KNOWN_SALT_MODELS = " | ".join((SALT_MONOVALENT, SALT_OWCZARZY_LITE, SALT_OWCZARZY08))

_CONC = re.compile(r"([+-]?(?:\d+\.?\d*|\.\d+)(?:e[+-]?\d+)?)\s*(\S+)")
_UNITS = {"m": 1.0, "mm": 1e-3, "um": 1e-6, "nm": 1e-9}


def ParseConc(s: str) -> float:
    """thermo.ParseConc -- conditions.go:128-155: "50mM", "250nM", "3uM", "3µM", "3μM" -> mol/L.  The reference scans a
    number and then a unit word (Sscanf "%f%s"), so a bare number is an error there and here."""
    raw = s.strip()
    norm = raw.lower().replace("µ", "u").replace("μ", "u")
    m = _CONC.match(norm)
    if not m:
        raise ValueError(f"invalid conc {_goq(raw)}: expected a number and a unit")
    val, unit = float(m.group(1)), m.group(2)
    if val < 0:
        raise ValueError(f"invalid conc {_goq(raw)}: concentration must be non-negative")
    if unit not in _UNITS:
        raise ValueError(f"unknown unit {_goq(unit)} in {_goq(raw)}")
    return val if unit == "m" else val * _UNITS[unit]


def _goq(s: str) -> str:
    import json
    return json.dumps(s, ensure_ascii=False)


def ParseSaltModel(raw: str) -> str:
    """thermo.ParseSaltModel -- conditions.go:57-68"""
    s = raw.strip().lower()
    if s == "":
        return SALT_MONOVALENT
    if s in (SALT_MONOVALENT, SALT_OWCZARZY_LITE, SALT_OWCZARZY08):
        return s
    raise ValueError(f"unknown salt model {_goq(raw)}; expected one of: {KNOWN_SALT_MODELS}")


def FreeMagnesium(mgM: float, dntpM: float) -> float:
    """conditions.go:172-190: free Mg2+ after dNTP chelation, Ka = 3e4 / M"""
    if mgM <= 0:
        return 0.0
    if dntpM <= 0:
        return mgM
    ka = 3e4
    b = ka * dntpM - ka * mgM + 1.0
    disc = b * b + 4.0 * ka * mgM
    if disc < 0 or math.isnan(disc) or math.isinf(disc):
        return 0.0
    free = (-b + math.sqrt(disc)) / (2.0 * ka)
    if free < 0 or math.isnan(free) or math.isinf(free):
        return 0.0
    return free


def EffectiveMonovalent(naM: float, mgM: float, dntpM: float, model: str) -> float:
    """conditions.go:159-167"""
    if (model or SALT_MONOVALENT) == SALT_OWCZARZY_LITE and mgM > 0:
        return naM + 3.8 * math.sqrt(FreeMagnesium(mgM, dntpM))
    return naM


@dataclass
class TmInput:
    """thermo.TmInput -- nn.go:64-71"""
    CT: float
    Na: float
    Mg: float = 0.0
    Dntp: float = 0.0
    SaltModel: str = SALT_MONOVALENT
    X: int = 4


@dataclass
class Conditions:
    """thermo.Conditions -- conditions.go:27-35 (zero = unset, as in the reference)"""
    AnnealC: float = 0.0
    NaM: float = 0.0
    MgM: float = 0.0
    DntpM: float = 0.0
    PrimerTotalM: float = 0.0
    SaltModel: str = ""
    SelfComplementary: bool = False

    def WithDefaults(self) -> "Conditions":                             # conditions.go:78-93 (MgM is not defaulted)
        d = DefaultConditions()
        return replace(self, AnnealC=self.AnnealC or d.AnnealC, NaM=self.NaM or d.NaM,
                       PrimerTotalM=self.PrimerTotalM or d.PrimerTotalM, SaltModel=self.SaltModel or d.SaltModel)

    def EffectiveNaM(self) -> float:
        c = self.WithDefaults()
        return EffectiveMonovalent(c.NaM, c.MgM, c.DntpM, c.SaltModel)

    def FreeMgM(self) -> float:
        c = self.WithDefaults()
        return FreeMagnesium(c.MgM, c.DntpM)

    def TmInput(self) -> TmInput:
        c = self.WithDefaults()
        return TmInput(CT=c.PrimerTotalM, Na=c.EffectiveNaM(), Mg=c.MgM, Dntp=c.DntpM, SaltModel=c.SaltModel,
                       X=1 if c.SelfComplementary else 4)


def DefaultConditions() -> Conditions:
    """the ipcr-thermo defaults, mol/L -- conditions.go:38-47"""
    return Conditions(AnnealC=60, NaM=0.05, MgM=0.003, DntpM=0, PrimerTotalM=2.5e-7, SaltModel=SALT_MONOVALENT)


# Watson-Crick stacks at 1 M Na+, top strand 5'->3' (dH kcal/mol, dS cal/(K mol)): the unified nearest-neighbour set
# (SantaLucia & Hicks 2004, table 1).  A stack and its strand-swapped reading are one duplex, so ten values fill sixteen keys.
_STACKS = {"AA": (-7.9, -22.2), "AT": (-7.2, -20.4), "TA": (-7.2, -21.3), "CA": (-8.5, -22.7), "GT": (-8.4, -22.4),
           "CT": (-7.8, -21.0), "GA": (-8.2, -22.2), "CG": (-10.6, -27.2), "GC": (-9.8, -24.4), "GG": (-8.0, -19.9)}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
for _k in list(_STACKS):
    _STACKS.setdefault(_COMP[_k[1]] + _COMP[_k[0]], _STACKS[_k])
_INIT, _TERM_AT, _SYMM = (0.2, -5.7), (2.2, 6.9), (0.0, -1.4)


@dataclass
class TmResult:
    """thermo.Result -- nn.go:74-79"""
    DH_kcal: float
    DS_cal: float
    DS_Na: float
    TmC: float


def _positive_salt(x: float) -> float:
    return 1e-9 if x <= 0 or math.isnan(x) or math.isinf(x) else x


def _gc_fraction(s: str) -> float:
    return sum(ch in "GC" for ch in s) / len(s) if s else 0.0


def Tm(primer5to3: str, target3to5: str, inp: TmInput) -> TmResult:
    """thermo.Tm -- nn.go:94-191: a perfect Watson-Crick duplex, primer 5'->3' on a target given 3'->5'; the three salt
    models.  ValueError where the reference returns an error."""
    p, t = primer5to3.strip().upper(), target3to5.strip().upper()
    if not p or not t or len(p) != len(t):
        raise ValueError("Tm: sequences must be equal length and non-empty")
    if inp.CT <= 0:
        raise ValueError("Tm: CT must be > 0")
    model = inp.SaltModel or SALT_MONOVALENT
    if inp.Na <= 0 and (model != SALT_OWCZARZY08 or FreeMagnesium(inp.Mg, inp.Dntp) <= 0):
        raise ValueError("Tm: salt concentration must be > 0")
    x = inp.X if inp.X in (1, 4) else 4
    if any(ch not in _COMP for ch in t):
        raise ValueError("Tm: non-ACGT base in target")
    for i, (a, b) in enumerate(zip(p, t)):
        if _COMP.get(a) != b:
            raise ValueError(f"Tm: non-WC pair at pos {i} ({a}/{b})")
    n = len(p)
    DH, DS = _INIT
    for i in range(n - 1):
        dh, ds = _STACKS[p[i:i + 2]]
        DH += dh
        DS += ds
    for end in (p[0], p[-1]):                                           # terminal AT, each end
        if end in "AT":
            DH += _TERM_AT[0]
            DS += _TERM_AT[1]
    if p == "".join(_COMP[ch] for ch in reversed(p)):                   # self-complementary
        DH += _SYMM[0]
        DS += _SYMM[1]
    N = float(2 * n - 2)
    log_conc = RCAL * math.log(inp.CT / float(x))
    DS_salt = DS + 0.368 * (N / 2.0) * math.log(_positive_salt(inp.Na))
    tmK = (DH * 1000.0) / (DS_salt + log_conc)
    if model == SALT_OWCZARZY08:
        tmK, DS_salt = _owczarzy08(DH, DS, log_conc, p, inp)
    return TmResult(DH, DS, DS_salt, tmK - 273.15)


def _owczarzy08(dh: float, ds: float, log_conc: float, primer: str, inp: TmInput):
    """nn.go:214-273: the 2008 mixed-salt correction as an inverse-temperature offset from the 1 M temperature, and the
    entropy that gives the same temperature back"""
    tm1 = (dh * 1000.0) / (ds + log_conc)
    free_mg = FreeMagnesium(inp.Mg, inp.Dntp)
    mon = _positive_salt(inp.Na)
    gc = _gc_fraction(primer)

    def mono_corr() -> float:
        ln = math.log(_positive_salt(mon))
        return (4.29 * gc - 3.95) * 1e-5 * ln + 9.40e-6 * ln * ln

    def mg_corr(mon_: float, ratio: float) -> float:
        ln_mg = math.log(_positive_salt(free_mg))
        a, b, c, d, e, f, g = 3.92, -0.911, 6.26, 1.42, -48.2, 52.5, 8.31
        if mon_ > 0 and ratio < 6.0:
            ln_mon = math.log(_positive_salt(mon_))
            sq = math.sqrt(_positive_salt(mon_))
            a = 3.92 * (0.843 - 0.352 * sq * ln_mon)
            d = 1.42 * (1.279 - 4.03e-3 * ln_mon - 8.03e-3 * ln_mon * ln_mon)
            g = 8.31 * (0.486 - 0.258 * ln_mon + 5.25e-3 * ln_mon * ln_mon * ln_mon)
        length = (e + f * ln_mg + g * ln_mg * ln_mg) / (2.0 * float(len(primer) - 1)) if len(primer) > 1 else 0.0
        return (a + b * ln_mg + gc * (c + d * ln_mg) + length) * 1e-5

    if free_mg <= 0:
        corr = mono_corr()
    else:                                                               # (mon > 0 always: _positive_salt)
        ratio = math.sqrt(free_mg) / mon
        corr = mono_corr() if ratio < 0.22 else mg_corr(mon, ratio)
    tmK = 1.0 / (1.0 / tm1 + corr)
    if math.isnan(tmK) or math.isinf(tmK) or tmK <= 0:
        return tmK, ds + 0.368 * (float(2 * len(primer) - 2) / 2.0) * math.log(_positive_salt(mon))
    return tmK, (dh * 1000.0) / tmK - log_conc


def score_conditions(cond: Conditions) -> Conditions:
    """Score.conditions() -- score.go:95-110, with the fields thermoapp fills (app.go:341-379): an unset NaM takes the
    effective monovalent value, then the defaults"""
    c = replace(cond)
    if c.NaM == 0:
        c.NaM = cond.EffectiveNaM()
    if c.SaltModel == "":
        c.SaltModel = SALT_MONOVALENT
    return c.WithDefaults()


def denom_for_primer(primer5to3: str, cond: Conditions) -> float:
    """Score.denomForPrimer -- score.go:465-492: |dS_Na + R ln(CT / X)| from the Tm of the primer on its own complement,
    X = 1 when the primer is its own reverse complement, else 4; 200.0 whenever that cannot be computed"""
    p = primer5to3.upper()
    if not p or any(ch not in _COMP for ch in p):
        return FIXED_DENOM
    c = score_conditions(cond)
    if c.NaM <= 0 or c.PrimerTotalM <= 0:
        return FIXED_DENOM
    comp = "".join(_COMP[ch] for ch in p)
    c.SelfComplementary = comp[::-1] == p
    inp = c.TmInput()
    try:
        res = Tm(p, comp, inp)
        D = res.DS_Na + RCAL * math.log(inp.CT / float(inp.X))
    except (ValueError, ZeroDivisionError, OverflowError):
        return FIXED_DENOM
    if math.isnan(D) or math.isinf(D) or D == 0:
        return FIXED_DENOM
    return -D if D < 0 else D


def panel_denoms(pairs: Sequence, cond: Optional[Conditions]) -> Optional[list]:
    """the table ipcr_thermo_legacy_products takes: D of pair p's forward / reverse primer at 2 p / 2 p + 1 (--denom
    auto); None for --denom fixed"""
    if cond is None:
        return None
    cache, out = {}, []
    for pr in pairs:
        for seq in (pr.Forward, pr.Reverse):
            if seq not in cache:
                cache[seq] = denom_for_primer(seq, cond)
            out.append(cache[seq])
    return out


@dataclass
class DuplexResult:
    """thermo.DuplexResult -- nn.go:81-88, the fields PerfectDuplex fills beside the Tm result"""
    Result: TmResult
    TmC: float
    AnnealC: float
    AnnealMarginC: float
    DeltaGAtAnnealKcal: float
    EffectiveDenomCalK: float
    SelfComplementary: bool


def PerfectDuplex(primer5to3: str, cond: Conditions) -> DuplexResult:
    """thermo.PerfectDuplex -- nn.go:279-301, of a primer on its own complement (what ImperfectDuplex anchors on,
    imperfect.go:264-268).  ValueError where the reference returns an error."""
    p = primer5to3.strip().upper()
    if not p or any(ch not in _COMP for ch in p):
        raise ValueError("PerfectDuplex: non-ACGT base in primer")
    comp = "".join(_COMP[ch] for ch in p)
    c = cond.WithDefaults()
    c.SelfComplementary = comp[::-1] == p
    inp = c.TmInput()
    res = Tm(p, comp, inp)
    denom = res.DS_Na + RCAL * math.log(inp.CT / float(inp.X))
    dg = res.DH_kcal - (c.AnnealC + 273.15) * denom / 1000.0
    return DuplexResult(res, res.TmC, c.AnnealC, res.TmC - c.AnnealC, dg, denom, c.SelfComplementary)


def nn_base_for_primer(primer5to3: str, cond: Conditions):
    """(tm_c, denom) of one primer for ipcr_thermo_nn_duplex_*: TmC and |EffectiveDenomCalK| of its perfect duplex, the
    denominator 200.0 when that is NaN, +-Inf or 0 (imperfect.go:273-276).  A primer that is not pure ACGT -- or whose Tm
    cannot be computed, where the reference returns an error for every product of it -- gets a finite placeholder: the
    library gives its ends status 1 in the first case; the second cannot arise from conditions score_conditions accepts."""
    try:
        d = PerfectDuplex(primer5to3, cond)
    except (ValueError, ZeroDivisionError, OverflowError):
        return 0.0, FIXED_DENOM
    denom = abs(d.EffectiveDenomCalK)
    if math.isnan(denom) or math.isinf(denom) or denom == 0:
        denom = FIXED_DENOM
    return (d.TmC if math.isfinite(d.TmC) else 0.0), denom


def panel_nn_base(pairs: Sequence, cond: Conditions) -> list:
    """the table ipcr_thermo_nn_duplex_products takes: (tm_c, denom) of pair p's forward / reverse primer at 2 p / 2 p + 1,
    under Score.conditions() (score_conditions) of `cond`; the anneal temperature that goes with it is
    score_conditions(cond).AnnealC"""
    c = score_conditions(cond)
    cache, out = {}, []
    for pr in pairs:
        for seq in (pr.Forward, pr.Reverse):
            if seq not in cache:
                cache[seq] = nn_base_for_primer(seq, c)
            out.append(cache[seq])
    return out


def nn_duplex_end(primer5to3: str, target3to5: str, dangling3p: str, tm_c: float, denom: float) -> "_lib.ThermoNNEnd":
    """ipcr_thermo_nn_duplex_end: one end on the host; dangling3p: the template base next to the primer's 3' end, "" for none"""
    out = _lib.ThermoNNEnd()
    d = dangling3p.encode("latin-1") if dangling3p else b"\0"
    _lib.check(_lib.lib().ipcr_thermo_nn_duplex_end(primer5to3.encode("latin-1"), target3to5.encode("latin-1"), d, float(tm_c),
                                                    float(denom), C.byref(out)))
    return out


def legacy_penalty(primer5to3: str, target3to5: str, denom: float = FIXED_DENOM) -> float:
    """ipcr_thermo_legacy_penalty: one end on the host"""
    out = C.c_double()
    _lib.check(_lib.lib().ipcr_thermo_legacy_penalty(primer5to3.encode("latin-1"), target3to5.encode("latin-1"), float(denom),
                                                     C.byref(out)))
    return out.value


def mismatch_ddg(p5: str, p: str, p3: str, t5: str, t: str, t3: str) -> float:
    """ipcr_thermo_mismatch_ddg (thermo.LookupDeltaG); IpcrError where the reference's look-up fails"""
    out = C.c_double()
    _lib.check(_lib.lib().ipcr_thermo_mismatch_ddg(*(x.encode("latin-1") for x in (p5, p, p3, t5, t, t3)), C.byref(out)))
    return out.value


def score_rank(score: float):
    """common.LessProductByScore -- sort.go:81-95 as the leading part of a sort key: higher scores first, NaN last; equal
    scores (and the NaNs among themselves) fall back to the coordinate order that follows in the key.  -0.0 == 0.0."""
    return (1, 0.0) if math.isnan(score) else (0, -score if score != 0 else 0.0)


def go_g(x: float) -> str:
    """Go's %g of a float64 (strconv.FormatFloat(x, 'g', -1, 64)): the shortest digits that read back as x; exponent form
    -- two exponent digits at least -- when the decimal exponent is below -4 or at least 6 (with shortest digits the
    format decides as if the precision were 6; 21 is encoding/json's bound, go_json_float); "-0" for negative zero"""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "+Inf" if x > 0 else "-Inf"
    if x == 0:
        return "-0" if math.copysign(1.0, x) < 0 else "0"
    sign, digits, exp = _shortest(x)
    if exp < -4 or exp >= 6:
        mant = digits[0] + ("." + digits[1:] if len(digits) > 1 else "")
        return f"{sign}{mant}e{'-' if exp < 0 else '+'}{abs(exp):02d}"
    return sign + _plain(digits, exp)


def go_json_float(x: float) -> str:
    """encoding/json's float64: plain digits unless |x| < 1e-6 or |x| >= 1e21, then exponent form with a one-digit
    exponent written without its leading zero"""
    if x == 0:
        return "-0" if math.copysign(1.0, x) < 0 else "0"
    sign, digits, exp = _shortest(x)
    if abs(x) < 1e-6 or abs(x) >= 1e21:
        mant = digits[0] + ("." + digits[1:] if len(digits) > 1 else "")
        return f"{sign}{mant}e{'-' if exp < 0 else '+'}{abs(exp)}"
    return sign + _plain(digits, exp)


def _shortest(x: float):
    """(sign, shortest round-trip digits without trailing zeros, decimal exponent of the first digit)"""
    m, e = ("%r" % abs(x)).partition("e")[::2] if "e" in repr(abs(x)) else (repr(abs(x)), "")
    ip, _, fp = m.partition(".")
    if fp == "0":
        fp = ""
    exp10 = int(e) if e else 0
    raw = ip + fp
    lead = len(raw) - len(raw.lstrip("0"))
    digits = raw.lstrip("0").rstrip("0") or "0"
    return ("-" if x < 0 else ""), digits, exp10 + len(ip) - 1 - lead


def _plain(digits: str, exp: int) -> str:
    if exp < 0:
        return "0." + "0" * (-exp - 1) + digits
    if len(digits) <= exp + 1:
        return digits + "0" * (exp + 1 - len(digits))
    return digits[:exp + 1] + "." + digits[exp + 1:]
