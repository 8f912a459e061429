! Test driver: a "host model" that diagnoses cloud cover from the sub-columns its radiation sees (module rrtmg_lw_cover) with the arrays
! of a stream file written by tests/test_fortran_cloud_cover.py.  Compiled with -cpp; -DWP=4 makes it a host built with 4-byte reals
! (the files always hold float64).  Two calls: every output (the packed mask with nsamp = 1 only), then cldtot alone by keyword.
!     drive_cloud_cover <in> <out>
#ifndef WP
#define WP 8
#endif
program drive_cloud_cover
  use iso_c_binding
  use parkind, only: im => kind_im
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_cover, only: rrtmg_lw_cloud_cover
  implicit none
  integer, parameter :: wp = WP, mw = 5
  integer(im) :: ncol, nlay, icld, seed, nsamp, seedstep, irng, irng2
  integer :: hdr(7), u
  real(8), allocatable :: play(:,:), cldfr(:,:), alpha(:,:)
  real(wp), allocatable :: hplay(:,:), hcldfr(:,:), halpha(:,:), cldtot(:), cldcum(:,:), cldlay(:,:), tot2(:)
  integer(c_int32_t), allocatable :: submask(:,:,:)
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr
  ncol = hdr(1); nlay = hdr(2); icld = hdr(3); seed = hdr(4); nsamp = hdr(5); seedstep = hdr(6); irng = hdr(7)
  allocate(play(ncol,nlay), cldfr(ncol,nlay), alpha(ncol,nlay))
  read(u) play, cldfr, alpha
  close(u)
  allocate(hplay(ncol,nlay), hcldfr(ncol,nlay), halpha(ncol,nlay), cldtot(ncol), cldcum(ncol,nlay), cldlay(ncol,nlay), tot2(ncol))
  allocate(submask(ncol,nlay,mw))
  hplay = real(play, wp); hcldfr = real(cldfr, wp); halpha = real(alpha, wp)
  cldtot = -1._wp; cldcum = -1._wp; cldlay = -1._wp; tot2 = -1._wp; submask = -1

  call rrtmg_lw_ini(1004.0_8)
  irng2 = irng
  if (nsamp == 1) then
     call rrtmg_lw_cloud_cover(ncol, nlay, icld, seed, nsamp, seedstep, irng, hplay, hcldfr, halpha, cldtot, cldcum, cldlay, submask)
  else
     call rrtmg_lw_cloud_cover(ncol, nlay, icld, seed, nsamp, seedstep, irng, hplay, hcldfr, halpha, cldtot, cldcum, cldlay)
  endif
  call rrtmg_lw_cloud_cover(ncol, nlay, icld, seed, nsamp, seedstep, irng2, hplay, hcldfr, alpha=halpha, cldtot=tot2)

  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) int(irng, 4), int(irng2, 4)
  write(u) real(cldtot, 8), real(cldcum, 8), real(cldlay, 8), real(tot2, 8)
  write(u) submask
  close(u)
end program drive_cloud_cover
