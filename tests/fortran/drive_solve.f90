! Test driver: a "host model" that forms its own optical depths and asks for the fluxes, with host arrays dimensioned (pcols, .),
! pcols = ncol + 3, through rrtmg_lw_solve (module rrtmg_lw_optics).  The output arrays hold NaN before the call; the driver counts
! what changed outside the call's columns.  Inputs and outputs travel through stream files written and read by
! tests/test_fortran_solve.py.
!     drive_solve <in> <out>
program drive_solve
  use iso_c_binding
  use ieee_arithmetic
  use parkind, only: im => kind_im
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_optics, only: rrtmg_lw_solve
  implicit none
  integer(im) :: ncol, nlay, cloud, idrv, ng, mw, pcols
  integer :: hdr(6), u, nbad, k
  real(8), allocatable :: plev(:,:), emis(:,:), tau(:,:,:), fracs(:,:,:), planklay(:,:,:), planklev(:,:,:), plankbnd(:,:), dplankbnd(:,:)
  real(8), allocatable :: cldfr(:,:), odcld(:,:,:)
  integer(c_int), allocatable :: submask(:,:,:)
  ! the same arrays dimensioned (pcols, .), and the outputs: levels (pcols,nlay+1,6) uflx, dflx, uflxc, dflxc, duflx_dt, duflxc_dt and
  ! layers (pcols,nlay,2) hr, hrc
  real(8), allocatable :: w_plev(:,:), w_emis(:,:), w_tau(:,:,:), w_fracs(:,:,:), w_play(:,:,:), w_plev16(:,:,:), w_pbnd(:,:), w_dpbnd(:,:)
  real(8), allocatable :: w_cldfr(:,:), w_odcld(:,:,:), o_lev(:,:,:), o_lay(:,:,:), x_lev(:,:,:), x_lay(:,:)
  integer(c_int), allocatable :: w_mask(:,:,:)
  real(8) :: nan
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr
  ncol = hdr(1); nlay = hdr(2); cloud = hdr(3); idrv = hdr(4); ng = hdr(5); mw = hdr(6)
  allocate(plev(ncol,nlay+1), emis(ncol,16), tau(ncol,nlay,ng), fracs(ncol,nlay,ng), planklay(ncol,nlay,16), planklev(ncol,nlay+1,16))
  allocate(plankbnd(ncol,16), dplankbnd(ncol,16), cldfr(ncol,nlay), odcld(ncol,nlay,16), submask(ncol,nlay,mw))
  read(u) plev, emis, tau, fracs, planklay, planklev, plankbnd, dplankbnd, cldfr, odcld, submask
  close(u)
  nan = ieee_value(nan, ieee_quiet_nan)
  call rrtmg_lw_ini(1004.0_8)

  ! ---- host arrays larger than the call (pcols > ncol): the rest holds NaN (the mask: all ones)
  pcols = ncol + 3
  allocate(w_plev(pcols,nlay+1), w_emis(pcols,16), w_tau(pcols,nlay,ng), w_fracs(pcols,nlay,ng), w_play(pcols,nlay,16), w_plev16(pcols,nlay+1,16))
  allocate(w_pbnd(pcols,16), w_dpbnd(pcols,16), w_cldfr(pcols,nlay), w_odcld(pcols,nlay,16), w_mask(pcols,nlay,mw))
  allocate(o_lev(pcols,nlay+1,6), o_lay(pcols,nlay,2), x_lev(ncol,nlay+1,2), x_lay(ncol,nlay))
  w_plev = nan; w_emis = nan; w_tau = nan; w_fracs = nan; w_play = nan; w_plev16 = nan; w_pbnd = nan; w_dpbnd = nan; w_cldfr = nan; w_odcld = nan
  w_mask = -1
  o_lev = nan; o_lay = nan
  w_plev(1:ncol,:) = plev; w_emis(1:ncol,:) = emis; w_tau(1:ncol,:,:) = tau; w_fracs(1:ncol,:,:) = fracs; w_play(1:ncol,:,:) = planklay
  w_plev16(1:ncol,:,:) = planklev; w_pbnd(1:ncol,:) = plankbnd; w_dpbnd(1:ncol,:) = dplankbnd; w_cldfr(1:ncol,:) = cldfr
  w_odcld(1:ncol,:,:) = odcld; w_mask(1:ncol,:,:) = submask
  if (idrv == 1) then
     call rrtmg_lw_solve(ncol, nlay, cloud, w_plev, w_emis, w_tau, w_fracs, w_play, w_plev16, w_pbnd, o_lev(:,:,1), o_lev(:,:,2), o_lay(:,:,1), &
                         uflxc=o_lev(:,:,3), dflxc=o_lev(:,:,4), hrc=o_lay(:,:,2), dplankbnd_dt=w_dpbnd, duflx_dt=o_lev(:,:,5), &
                         duflxc_dt=o_lev(:,:,6), cldfr=w_cldfr, odcld=w_odcld, submask=w_mask)
  else
     call rrtmg_lw_solve(ncol, nlay, cloud, w_plev, w_emis, w_tau, w_fracs, w_play, w_plev16, w_pbnd, o_lev(:,:,1), o_lev(:,:,2), o_lay(:,:,1), &
                         uflxc=o_lev(:,:,3), dflxc=o_lev(:,:,4), hrc=o_lay(:,:,2), cldfr=w_cldfr, odcld=w_odcld, submask=w_mask)
     o_lev(1:ncol,:,5:6) = 0.0_8
  endif
  ! ... and the required outputs alone, exactly sized
  call rrtmg_lw_solve(ncol, nlay, cloud, plev, emis, tau, fracs, planklay, planklev, plankbnd, x_lev(:,:,1), x_lev(:,:,2), x_lay, &
                      cldfr=cldfr, odcld=odcld, submask=submask)
  nbad = count(.not. ieee_is_nan(o_lev(ncol+1:,:,:))) + count(.not. ieee_is_nan(o_lay(ncol+1:,:,:)))
  if (any(x_lev(:,:,1) /= o_lev(1:ncol,:,1)) .or. any(x_lev(:,:,2) /= o_lev(1:ncol,:,2)) .or. any(x_lay /= o_lay(1:ncol,:,1))) nbad = nbad + 1000000

  ! nbad, 0; uflx, dflx, uflxc, dflxc, duflx_dt, duflxc_dt; hr, hrc
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) nbad, 0
  do k = 1, 6
     write(u) o_lev(1:ncol,:,k)
  enddo
  write(u) o_lay(1:ncol,:,1), o_lay(1:ncol,:,2)
  close(u)
end program drive_solve
