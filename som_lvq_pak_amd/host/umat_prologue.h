/* umat_prologue.h -- the PostScript prologue umat writes between %%EndComments and its "/radius ... def" line.
 *
 * This project's own: the body that follows (written by umat.c in SOM_PAK's format, byte for byte) only needs the names
 * below to exist with these meanings.  The prologue opens one dictionary, which the body's final `end` closes, and
 * pre-defines every name the body redefines.
 *   XSR         start a row at (xoff, yoff)
 *   XSH         the same for hexagonal rows: shifted right by xstep/2 when y mod 4 is 1 or 3, by xstep when it is 2
 *   NL          next row: yoff goes down by ystep, y counts up
 *   v H, v R    a hexagon of `radius` / a square of side xstep at the current point, filled with grey level v (0..100,
 *               rescaled between bt and wt), outlined in the contrasting colour when doborder; advance by xstep
 *   v LN        a dot;  (s) v LAB  a centred label;  (s1)...(sn) n v ML  n stacked centred labels -- black or white,
 *               whichever contrasts with v; advance by 2 xstep
 *   selfont     select fontname at fontsize (relative to radius);  swapx, swapy  mirror the picture
 * A user who wants SOM_PAK's own picture passes its header with -headerfile (or UMAT_HEADERFILE).
 * One C string per line; no PostScript strings inside and comments only as whole lines (tests/test_umat.py counts
 * braces and names).  No PostScript interpreter checks it automatically: see DESIGN.md. */
static const char *const umat_prologue[] = {
  "%%BeginProlog\n",
  "64 dict begin\n",
  "/xstep 10 def /ystep 10 def /radius 5 def\n",
  "/xoff 0 def /yoff 0 def /y 0 def\n",
  "/xoffset 0 def /yoffset 0 def\n",
  "/picwidth 1000 def /picheight 1000 def\n",
  "/doborder false def /fontname /Helvetica def /fontsize 1.0 def /bt 0 def /wt 1 def\n",
  "/v 0 def /n 0 def /k 0 def /cx 0 def /cy 0 def /side 0 def /lh 0 def\n",
  "/selfont { fontname findfont fontsize radius mul scalefont setfont } def\n",
  "/swapx { /xstep xstep neg def /xoffset picwidth xoffset sub def } def\n",
  "/swapy { /ystep ystep neg def /yoffset picheight yoffset sub def } def\n",
  "/XSR { xoff yoff moveto } def\n",
  "/XSH { xoff y 4 mod dup dup 1 eq exch 3 eq or\n",
  "  { pop xstep 2 div add } { 2 eq { xstep add } if } ifelse yoff moveto } def\n",
  "/NL { /yoff yoff ystep sub def /y y 1 add def } def\n",
  "/unit01 { dup 0 lt { pop 0 } if dup 1 gt { pop 1 } if } def\n",
  "/GL { 100 div unit01 bt sub wt bt sub dup 0 eq { pop 1 } if div unit01 } def\n",
  "/CC { GL 0.5 lt { 1 } { 0 } ifelse } def\n",
  "/here { currentpoint /cy exch def /cx exch def } def\n",
  "/paint { gsave v GL setgray fill grestore\n",
  "  doborder { v CC setgray radius 20 div setlinewidth stroke } { newpath } ifelse } def\n",
  "/H { /v exch def here newpath cx cy radius add moveto\n",
  "  1 1 5 { 60 mul 90 add dup cos radius mul cx add exch sin radius mul cy add lineto } for closepath\n",
  "  paint cx xstep add cy moveto } def\n",
  "/R { /v exch def here /side xstep abs def newpath cx side 2 div sub cy side 2 div sub moveto\n",
  "  side 0 rlineto 0 side rlineto side neg 0 rlineto closepath\n",
  "  paint cx xstep add cy moveto } def\n",
  "/LN { CC setgray here newpath cx cy radius 6 div 0 360 arc fill cx xstep 2 mul add cy moveto } def\n",
  "/centred { dup stringwidth pop 2 div neg cx add 3 -1 roll moveto show } def\n",
  "/LAB { CC setgray here /lh fontsize radius mul def cy lh 3 div sub exch centred\n",
  "  cx xstep 2 mul add cy moveto } def\n",
  "/ML { CC setgray /n exch def here /lh fontsize radius mul def\n",
  "  0 1 n 1 sub { /k exch def k n 1 sub 2 div sub lh mul cy add lh 3 div sub exch centred } for\n",
  "  cx xstep 2 mul add cy moveto } def\n",
  "%%EndProlog\n",
  0
};
